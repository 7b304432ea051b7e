"""ctypes binding of liblpf.so (include/lpf.h) -- the only route to the hot path.

There is no CPU fallback: if the HIP library is missing or no GPU is present the
calls raise.  NumPy arrays go through the ABI's host-pointer mode; torch CUDA (ROCm)
tensors are passed by ``data_ptr()`` in device mode.
"""
import collections
import ctypes
import os
import sys
import weakref

import numpy as np

from . import _build
from .idmap import IdMasks
from .rle import RleMasks

LPF_MAX_MASKS = 32
LPF_ASSIGN_MAX = 1024             # rows and live columns of a frame of lpf_assign_costs / lpf_assign_2d
LPF_MAX_MASKS_WIDE = 256                # lpf_run_wide: masks per frame in one pass
_P = ctypes.c_void_p
_I64 = ctypes.c_int64


class LpfError(RuntimeError):
    """An lpf_* call returned a negative status (message from lpf_last_error)."""

    def __init__(self, code, msg):
        super().__init__("liblpf error %d: %s" % (code, msg))
        self.code = code


class FrameSummary(ctypes.Structure):
    _fields_ = [("n_valid", _I64), ("n_labelled", _I64),
                ("inst_count", _I64 * LPF_MAX_MASKS), ("inst_off", _I64 * (LPF_MAX_MASKS + 1)),
                ("best_cnt", _I64 * LPF_MAX_MASKS), ("best_box", ctypes.c_int32 * LPF_MAX_MASKS),
                ("inst_overflow", ctypes.c_int32), ("reserved", ctypes.c_int32)]


SUMMARY_DTYPE = np.dtype([("n_valid", "<i8"), ("n_labelled", "<i8"), ("inst_count", "<i8", (32,)),
                          ("inst_off", "<i8", (33,)), ("best_cnt", "<i8", (32,)), ("best_box", "<i4", (32,)),
                          ("inst_overflow", "<i4"), ("reserved", "<i4")])
assert SUMMARY_DTYPE.itemsize == ctypes.sizeof(FrameSummary) == 928


class Outputs(ctypes.Structure):
    _fields_ = [("uv", _P), ("label_bits", _P), ("depth", _P), ("u_f", _P), ("v_f", _P),
                ("valid_idx", _P), ("inst_idx", _P), ("inst_cap", _I64), ("count_mb", _P),
                ("summary", _P), ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("uv_valid", _P), ("label_valid", _P)]


class WideInput(ctypes.Structure):
    """lpf_wide_input (include/lpf.h): the masks of an lpf_run_wide call"""
    _fields_ = [("masks", _P), ("rects", _P), ("M", ctypes.c_int32), ("f32", ctypes.c_int32), ("binarize", ctypes.c_int32),
                ("erode_iters", ctypes.c_int32), ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class RleMasksInput(ctypes.Structure):
    """lpf_rle_masks (include/lpf.h): the run-length masks of an lpf_set_masks_rle call"""
    _fields_ = [("runs", _P), ("run_off", _P), ("F", ctypes.c_int32), ("M", ctypes.c_int32), ("erode_iters", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]

    @classmethod
    def of(cls, runs, run_off, F, M, erode_iters=0):
        """The struct over rle_batch's tables (which must stay alive as long as it is used)"""
        return cls(runs.ctypes.data if len(runs) else None, run_off.ctypes.data, F, M, int(erode_iters), 0)


class IdMasksInput(ctypes.Structure):
    """lpf_id_masks (include/lpf.h): the instance-ID maps of an lpf_set_masks_ids / lpf_run_wide_ids call"""
    _fields_ = [("ids", _P), ("sel", _P), ("F", ctypes.c_int32), ("M", ctypes.c_int32), ("id_bytes", ctypes.c_int32),
                ("erode_iters", ctypes.c_int32), ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class WideOutputs(ctypes.Structure):
    """lpf_wide_outputs (include/lpf.h)"""
    _fields_ = [("uv", _P), ("depth", _P), ("u_f", _P), ("v_f", _P), ("valid_idx", _P), ("uv_valid", _P), ("label_words", _P),
                ("label_valid_words", _P), ("inst_idx", _P), ("inst_cap", _I64), ("count_mb", _P), ("n_valid", _P), ("n_labelled", _P),
                ("inst_count", _P), ("inst_off", _P), ("best_cnt", _P), ("best_box", _P), ("inst_overflow", _P),
                ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class DepthMapsOutputs(ctypes.Structure):
    """lpf_depth_maps_outputs (include/lpf.h): the per-car sparse depth maps of an lpf_depth_maps call"""
    _fields_ = [("pix", _P), ("depth", _P), ("point_idx", _P), ("cap", _I64), ("car_off", _P), ("need", _P), ("overflow", _P),
                ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class DepthOverlayInput(ctypes.Structure):
    """lpf_depth_overlay_input (include/lpf.h): the sparse lists of lpf_depth_maps and the segmented images of an lpf_depth_overlays call"""
    _fields_ = [("pix", _P), ("depth", _P), ("cap", _I64), ("car_off", _P), ("M", ctypes.c_int32), ("lists_on_device", ctypes.c_int32),
                ("seg", _P), ("seg_on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class DepthOverlayOutputs(ctypes.Structure):
    """lpf_depth_overlay_outputs (include/lpf.h): the per-car overlay images and np.max of each car's depth map"""
    _fields_ = [("images", _P), ("max_depth", _P), ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Match2dInput(ctypes.Structure):
    """lpf_match2d_input (include/lpf.h): the detections and projected boxes of a batch of frames for lpf_match_2d"""
    _fields_ = [("dets", _P), ("det_off", _P), ("bbox2d", _P), ("front", _P), ("box_off", _P), ("dets_f64", ctypes.c_int32),
                ("on_device", ctypes.c_int32), ("min_iou", ctypes.c_double), ("w_iou", ctypes.c_double), ("w_center", ctypes.c_double),
                ("w_size", ctypes.c_double)]


class Match2dOutputs(ctypes.Structure):
    """lpf_match2d_outputs (include/lpf.h): V4's choice per detection and V5's score matrices per pair"""
    _fields_ = [("best_box", _P), ("best_iou", _P), ("iou", _P), ("center_score", _P), ("size_score", _P), ("total_score", _P),
                ("cost", _P), ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AssignInput(ctypes.Structure):
    """lpf_assign_input (include/lpf.h): the cost matrices of a batch of frames for lpf_assign_costs"""
    _fields_ = [("cost", _P), ("det_off", _P), ("box_off", _P), ("front", _P), ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AssignOutputs(ctypes.Structure):
    """lpf_assign_outputs (include/lpf.h): the column of every row and the status of every frame"""
    _fields_ = [("col_of_row", _P), ("status", _P), ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Assign2dParams(ctypes.Structure):
    """lpf_assign2d_params (include/lpf.h): V5's two acceptance thresholds"""
    _fields_ = [("min_score_threshold", ctypes.c_double), ("min_iou_threshold", ctypes.c_double)]


class Assign2dOutputs(ctypes.Structure):
    """lpf_assign2d_outputs (include/lpf.h): per detection its box, the four scores of that pair and accepted or not"""
    _fields_ = [("box_of_det", _P), ("iou", _P), ("center_score", _P), ("size_score", _P), ("total_score", _P), ("accepted", _P),
                ("status", _P), ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class InsideInput(ctypes.Structure):
    """lpf_inside_input (include/lpf.h): a run's instance lists and best boxes, for lpf_inside_masks"""
    _fields_ = [("inst_idx", _P), ("inst_cap", _I64), ("inst_off", _P), ("best_box", _P), ("best_cnt", _P), ("M", ctypes.c_int32),
                ("min_points", ctypes.c_int32), ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class InsideOutputs(ctypes.Structure):
    """lpf_inside_outputs (include/lpf.h): per list entry the inside byte and the inside-first partition, per car the counts"""
    _fields_ = [("inside", _P), ("part_idx", _P), ("part_xyz", _P), ("n_inside", _P), ("matched", _P), ("on_device", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class BoxPointsInput(ctypes.Structure):
    """lpf_box_points_input (include/lpf.h): a run's compact valid indices and label words, for lpf_box_points"""
    _fields_ = [("valid_idx", _P), ("n_valid", _P), ("label_valid_words", _P), ("LW", ctypes.c_int32), ("on_device", ctypes.c_int32)]


class BoxPointsOutputs(ctypes.Structure):
    """lpf_box_points_outputs (include/lpf.h): per box the valid points it holds, per valid point its first box, per frame four counts"""
    _fields_ = [("box_points", _P), ("box_labelled", _P), ("first_box", _P), ("frame_counts", _P), ("on_device", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class FirstMatchInput(ctypes.Structure):
    """lpf_first_match_input (include/lpf.h): the masks of a batch at their own size and the colour rows car_rgb gathers"""
    _fields_ = [("masks", _P), ("colors", _P), ("M", ctypes.c_int32), ("mh", ctypes.c_int32), ("mw", ctypes.c_int32), ("f32", ctypes.c_int32),
                ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class FirstMatchRleInput(ctypes.Structure):
    """lpf_first_match_rle_input (include/lpf.h): a batch's run-length masks at their own size and the colour rows car_rgb gathers"""
    _fields_ = [("masks", ctypes.POINTER(RleMasksInput)), ("colors", _P), ("mh", ctypes.c_int32), ("mw", ctypes.c_int32),
                ("colors_on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class FirstMatchOutputs(ctypes.Structure):
    """lpf_first_match_outputs (include/lpf.h): the dense first-mask codes, the compact car and background lists, the counts"""
    _fields_ = [("first_mask", _P), ("car_idx", _P), ("car_mask", _P), ("car_xyz", _P), ("car_rgb", _P), ("bg_idx", _P), ("bg_xyz", _P),
                ("n_valid", _P), ("n_car", _P), ("n_bg", _P), ("mask_count", _P), ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class BoxViewsInput(ctypes.Structure):
    """lpf_box_views_input (include/lpf.h): the cam-0 corners of a batch of frames' boxes and the filter's thresholds"""
    _fields_ = [("corners_cam0", _P), ("box_off", _P), ("T_cam_to_velo", _P), ("on_device", ctypes.c_int32),
                ("min_points_in_view", ctypes.c_int32), ("depth_lo", ctypes.c_double), ("depth_hi", ctypes.c_double),
                ("min_area", ctypes.c_double)]


class BoxViewsOutputs(ctypes.Structure):
    """lpf_box_views_outputs (include/lpf.h): per box the filter's verdict and V5's projection, per frame the counts per reason"""
    _fields_ = [("keep", _P), ("reason", _P), ("corners_in_view", _P), ("corners_near", _P), ("avg_depth", _P), ("near_bbox2d", _P),
                ("front", _P), ("bbox2d", _P), ("front_avg_depth", _P), ("kept_pos", _P), ("frame_counts", _P), ("corners_velo", _P),
                ("on_device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


LPF_MAX_CAMS = 4                        # lpf_run_cams / lpf_run_cams_wide: cameras of one pass


class CamInput(ctypes.Structure):
    """lpf_cam_input (include/lpf.h): one camera of an lpf_run_cams pass"""
    _fields_ = [("T_velo_to_rect", ctypes.c_double * 16), ("K", ctypes.c_double * 9), ("W", ctypes.c_int32), ("H", ctypes.c_int32),
                ("depth_min_excl", ctypes.c_double), ("depth_max_excl", ctypes.c_double), ("masks", WideInput),
                ("corners_velo", _P), ("box_off", _P), ("boxes_on_device", ctypes.c_int32), ("oriented", ctypes.c_int32)]


# A pass's masks, checked (wide_mask_batch, compact_mask_batch).  form "dense": ``masks`` [F,M,H,W], ``is_float``, ``rects`` [F,M,4] or
# None.  form "rle" / "ids" (a row of MASK_FORMS): ``struct`` is the form's ctypes struct as the native calls take it and ``tables`` the
# two arrays it points into, which must stay alive as long as it is used; ``masks`` and ``rects`` are None.  gpu: a tensor of the inputs
# when they are GPU memory (``on_device``) -- a call that reads them waits for the stream that made them -- else None.
MaskBatch = collections.namedtuple("MaskBatch", "masks M is_float on_device rects form struct tables gpu",
                                   defaults=("dense", None, None, None))


def _check_erode_iters(erode_iters):
    """The erosion count of a checked batch and of set_masks_ids (set_masks_rle keeps a looser check of its own)"""
    if int(erode_iters) != erode_iters or erode_iters < 0:
        raise ValueError("erode_iters must be a non-negative integer, got %r" % (erode_iters,))


def wide_mask_batch(masks, F, H, W, rects=None, erode_iters=0, binarize="astype", binarize_codes=None):
    """Checks the masks of a wide run before anything reaches the GPU: MaskBatch ``(masks [F,M,H,W], M, is_float, on_device, rects
    [F,M,4] or None)``.  masks: [M,H,W] (F = 1) or [F,M,H,W], uint8 / bool or float32, a NumPy array or a contiguous GPU tensor; M <= 256."""
    codes = binarize_codes or {"astype": 0, "v3": 1, "gt0.5": 2}
    if binarize not in codes:
        raise ValueError("binarize must be one of %s" % sorted(codes))
    _check_erode_iters(erode_iters)
    dev = _is_torch(masks)
    if not dev:
        masks = np.asarray(masks)
    shape = tuple(masks.shape)
    if len(shape) == 3:
        shape = (1,) + shape
        masks = masks.reshape(shape)
    if len(shape) != 4 or shape[0] != F or (shape[1] and shape[2:] != (H, W)):
        raise ValueError("masks must be [M,%d,%d] (one frame) or [F=%d,M,%d,%d], got %s" % (H, W, F, H, W, tuple(masks.shape)))
    M = shape[1]
    if M > LPF_MAX_MASKS_WIDE:
        raise ValueError("at most %d masks per frame in one wide run, got %d" % (LPF_MAX_MASKS_WIDE, M))
    if dev:
        dt = str(masks.dtype)
        if dt not in ("torch.float32", "torch.uint8", "torch.bool") or not masks.is_cuda or not masks.is_contiguous():
            raise ValueError("device masks must be contiguous float32, uint8 or bool GPU tensors")
        is_f = dt == "torch.float32"
    else:
        if masks.dtype.kind not in "fbiu":
            raise ValueError("masks must be numeric, got %s" % masks.dtype)
        is_f = masks.dtype.kind == "f"
        masks = np.ascontiguousarray(masks, dtype=np.float32 if is_f else np.uint8)
    if rects is not None:
        if _is_torch(rects) != dev:
            raise ValueError("the rectangles must live where the masks do")
        rshape = tuple(rects.shape)
        if len(rshape) == 2:
            rshape = (1,) + rshape
        if rshape != (F, M, 4):
            raise ValueError("rects must be [F=%d, M=%d, 4], got %s" % (F, M, tuple(rects.shape)))
        if dev:
            if str(rects.dtype) != "torch.int32" or not rects.is_contiguous():
                raise ValueError("device rects must be a contiguous int32 tensor")
        else:
            rects = np.ascontiguousarray(np.asarray(rects).reshape(rshape), dtype=np.int32)
    return MaskBatch(masks, M, is_f, dev, rects, gpu=masks if dev else None)


LPF_MASKS_U8, LPF_MASKS_F32, LPF_MASKS_RLE = 0, 1, 2           # lpf_wide_input.f32 (include/lpf.h)


def ids_batch(frames_masks, H, W, max_masks=LPF_MAX_MASKS, who="set_masks_ids"):
    """``(maps, sel int32 [F,M], F, M, id_bytes, on_device)`` of one IdMasks or a list of them, one per frame, as lpf_set_masks_ids -- or
    lpf_run_wide_ids, with ``max_masks`` = 256 -- takes them.  Frames with fewer masks than the largest are padded with LPF_ID_NONE.
    Host maps are stacked into ONE [F,H,W] array; GPU maps must already be the frames of one contiguous [F,H,W] tensor (``IdMasks(t[f],
    ...)``), or F = 1: ``maps`` is then the first frame's tensor.  ValueError -- before any native call, with ``who`` as the message's
    prefix -- for anything that is not an IdMasks, another size than H x W, more than max_masks masks, differing ID dtypes, host and
    GPU maps in one call, and GPU maps that are not contiguous or do not follow one another in memory."""
    from .idmap import LPF_ID_NONE, check_sel
    frames = [frames_masks] if isinstance(frames_masks, IdMasks) else list(frames_masks)
    for f, r in enumerate(frames):
        if not isinstance(r, IdMasks):
            raise ValueError("%s: frame %d is %s, not IdMasks" % (who, f, type(r).__name__))
        if tuple(r.shape[1:]) != (H, W):
            raise ValueError("%s: frame %d has a map of %d x %d, the camera is %d x %d (maps are not resized)"
                             % (who, f, r.shape[2], r.shape[1], W, H))
        if r.shape[0] > max_masks:
            raise ValueError("%s: frame %d has %d masks, one pass takes %d (pipeline.run_frames groups them)"
                             % (who, f, r.shape[0], max_masks))
    F = len(frames)
    M = max([r.shape[0] for r in frames], default=0)
    sel = np.full((F, M), LPF_ID_NONE, np.int32)
    for f, r in enumerate(frames):
        sel[f, :r.shape[0]] = check_sel(r.sel, "%s: frame %d" % (who, f))     # (checked again: the fields of an IdMasks can be assigned)
    if F == 0:
        return None, sel, 0, M, 2, False
    dts = {np.dtype(r.id_dtype) for r in frames}
    if len(dts) != 1:
        raise ValueError("%s: the frames' maps have differing ID dtypes %s: one dtype per call" % (who, sorted(d.name for d in dts)))
    dt = dts.pop()
    dev = [r.on_device for r in frames]
    if any(dev) != all(dev):
        raise ValueError("%s: host and GPU maps in one call: one place per call" % who)
    if not dev[0]:
        maps = np.ascontiguousarray(frames[0].ids[None] if F == 1 else np.stack([r.ids for r in frames]), dtype=dt)
        return maps, sel, F, M, dt.itemsize, False
    t0 = frames[0].ids
    for f, r in enumerate(frames):
        if not r.ids.is_cuda or not r.ids.is_contiguous() or r.ids.data_ptr() != t0.data_ptr() + f * H * W * dt.itemsize:
            raise ValueError("%s: GPU maps must be the frames of ONE contiguous [F,H,W] tensor (IdMasks(t[f], sel)), or F = 1: frame %d "
                             "is not where frame 0 + %d frames is" % (who, f, f))
    return [r.ids for r in frames], sel, F, M, dt.itemsize, True


def _ids_input(maps, sel, F, M, id_bytes, on_device, erode_iters):
    """The lpf_id_masks over ids_batch's arrays (which must stay alive as long as it is used)"""
    if F == 0:
        ptr = None
    elif on_device:
        ptr = maps[0].data_ptr()
    else:
        ptr = maps.ctypes.data
    return IdMasksInput(ptr, sel.ctypes.data if sel.size else None, F, M, id_bytes, int(erode_iters), 1 if on_device else 0, 0)


# The compact forms of masks, one row each: the class a caller hands over (its name is the word the refusals use), the two texts the
# forms' refusals differ by, ``batch(frames, H, W, max_masks, who)`` -- a list of them as the tables of one call, (two arrays, F, M,
# ...) -- and ``struct(*that tuple, erode_iters)``, the ctypes struct over the tables.  An entry point names the forms it takes
# (``forms=``); a form it does not take is not recognised there and goes the dense way, to that path's own refusal.
MaskForm = collections.namedtuple("MaskForm", "name cls where mixes batch struct")
MASK_FORMS = (
    MaskForm("rle", RleMasks, "the runs say where the masks are",
             "the list mixes RleMasks and arrays: one form per call (.to_dense() or RleMasks.from_dense)",
             lambda *a: LpfContext.rle_batch(*a), RleMasksInput.of),
    MaskForm("ids", IdMasks, "the map says where the masks are",
             "the list mixes IdMasks with another form of masks: one form per call (.to_dense())", ids_batch, _ids_input))


def compact_frames(masks, who, forms):
    """Is this ``masks`` argument in one of the compact ``forms`` (names of MASK_FORMS, tried in that order) -- one instance of the
    form's class, or a list with one per frame?  ``(the form's row, the per-frame list)``, or None for anything else; ValueError
    (``who``: the message's prefix) for a list that mixes the form with anything else."""
    frames = list(masks) if isinstance(masks, (list, tuple)) else [masks]
    for form in (f for name in forms for f in MASK_FORMS if f.name == name):
        if any(isinstance(m, form.cls) for m in frames):
            if not all(isinstance(m, form.cls) for m in frames):
                raise ValueError("%s: %s" % (who, form.mixes))
            return form, frames
    return None


def compact_mask_batch(masks, F, H, W, rects=None, erode_iters=0, binarize="astype", max_masks=LPF_MAX_MASKS_WIDE, who="run_wide",
                       default_binarize="astype", *, forms):
    """A compact form of a pass's masks -- one rle.RleMasks or idmap.IdMasks, or a list with one per frame -- checked before anything
    reaches the GPU: a MaskBatch of that form; None when ``masks`` are in none of ``forms``.  Ragged M is padded (empty masks,
    LPF_ID_NONE).  ValueError: a list that mixes the form with anything else, ``rects`` (the form needs none), a ``binarize`` other than
    the entry point's default (``default_binarize``), what the form's batch builder refuses (rle_batch, ids_batch: another size than
    H x W, more than max_masks masks, ...), another frame count than F."""
    found = compact_frames(masks, who, forms)
    if found is None:
        return None
    form, frames = found
    noun = form.cls.__name__
    if rects is not None:
        raise ValueError("%s: rects given with %s (%s)" % (who, noun, form.where))
    if binarize != default_binarize:
        raise ValueError("%s: binarize=%r with %s (a pixel is a member or it is not)" % (who, binarize, noun))
    _check_erode_iters(erode_iters)
    tables = form.batch(frames, H, W, max_masks, who)
    if tables[2] != F:
        raise ValueError("%s: %s for %d frames, the batch has %d" % (who, noun, tables[2], F))
    struct = form.struct(*tables, erode_iters)
    gpu = tables[0][0] if getattr(struct, "on_device", 0) else None      # (GPU maps: the frames' tensors; runs are host memory)
    return MaskBatch(None, tables[3], False, gpu is not None, None, form.name, struct, tables[:2], gpu)


class FrameJob(ctypes.Structure):
    """lpf_frame_job (include/lpf.h): one frame of a stream -- scan, masks + rectangles, cam-0 box corners, outputs -- for lpf_run_frame"""
    _fields_ = [("pts", _P), ("n_points", _I64), ("masks", _P), ("mask_rects", _P), ("corners_cam0", _P), ("T_cam_to_velo", _P),
                ("n_masks", ctypes.c_int32), ("n_boxes", ctypes.c_int32), ("filter_visible", ctypes.c_int32), ("oriented", ctypes.c_int32),
                ("out", Outputs)]


class FrameJobWide(ctypes.Structure):
    """lpf_frame_job_wide (include/lpf.h): one frame of a stream with up to 256 masks -- scan, lent uint8 masks + rectangles, cam-0
    box corners, wide outputs -- for lpf_run_frame_wide"""
    _fields_ = [("pts", _P), ("n_points", _I64), ("masks", _P), ("mask_rects", _P), ("corners_cam0", _P), ("T_cam_to_velo", _P),
                ("n_masks", ctypes.c_int32), ("n_boxes", ctypes.c_int32), ("filter_visible", ctypes.c_int32), ("oriented", ctypes.c_int32),
                ("out", WideOutputs)]


_libs = {}


def library_path():
    """liblpf.so of this package.  LPF_LIBRARY names another build of the same ABI, and is honoured ONLY in lab runs (LPF_LAB=1 in the
    environment, which `bench.py --lab ...` and the tools set): a stray variable must not silently swap the library a number or a
    test is made with."""
    env = os.environ.get("LPF_LIBRARY")
    if env:
        if os.environ.get("LPF_LAB") != "1":
            raise LpfError(-3, "LPF_LIBRARY=%s is set but this is not a lab run (LPF_LAB=1; bench.py --lab ...): refusing to load another "
                               "library in place of %s" % (env, _build.LIB))
        return env
    return _build.LIB


def _own(path):
    """lab flag if `path` is one of this package's two libraries (they are tied to the sources beside them), else None"""
    for lib, lab in ((_build.LIB, False), (_build.LAB_LIB, True)):
        if os.path.abspath(path) == os.path.abspath(lib):
            return lab
    return None


def load(path=None):
    """dlopen liblpf.so (or another build of the same ABI at ``path``).  The package's own libraries are tied to their sources: a
    missing or STALE one (its compiled-in build id differs from _build.source_id()) is rebuilt with hipcc, and refused if that is
    not possible -- never loaded as it is, and there is no CPU path to fall back to."""
    path = os.path.abspath(path or library_path())
    if path in _libs:
        return _libs[path]
    lab = _own(path)
    if lab is not None and _build.needs_build(path):
        have = _build.library_id(path)
        try:
            import fcntl
            with open(path + ".lock", "w") as lk:           # (the ranks of a multi-process run must not rebuild the file under each other)
                fcntl.flock(lk, fcntl.LOCK_EX)
                if _build.needs_build(path):
                    _build.build(lab=lab)
        except Exception as e:
            raise LpfError(-2, "%s is %s and cannot be rebuilt here (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(hipcc --offload-arch=gfx950); there is no CPU path" % (
                                   path, "missing" if not os.path.exists(path) else "stale (built from sources %s, these are %s)" % (have, _build.source_id(lab)), e))
    if not os.path.exists(path):
        raise LpfError(-2, "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU path" % path)
    lib = ctypes.CDLL(path)
    build_id = None
    if hasattr(lib, "lpf_build_id"):
        lib.lpf_build_id.restype = ctypes.c_char_p
        build_id = (lib.lpf_build_id() or b"").decode()
    if lab is not None and build_id != _build.source_id(lab):
        raise LpfError(-2, "%s reports build id %s, the sources beside it are %s: refusing a library that is not built from them" % (
            path, build_id, _build.source_id(lab)))
    lib._lpf_info = {"path": path, "build_id": build_id}
    if hasattr(lib, "lpf_host_alloc"):
        lib.lpf_host_alloc.restype = _P
        lib.lpf_host_alloc.argtypes = [ctypes.c_size_t]
        lib.lpf_host_free.restype = None
        lib.lpf_host_free.argtypes = [_P]
    lib.lpf_last_error.restype = ctypes.c_char_p
    lib.lpf_last_error.argtypes = [_P]
    lib.lpf_create.argtypes = [ctypes.POINTER(_P), ctypes.c_int]
    lib.lpf_destroy.argtypes = [_P]
    lib.lpf_destroy.restype = None
    lib.lpf_set_stream.argtypes = [_P, _P]
    lib.lpf_use_own_stream.argtypes = [_P]
    lib.lpf_wait_for_stream.argtypes = [_P, _P]
    lib.lpf_release_to_stream.argtypes = [_P, _P]
    lib.lpf_sync.argtypes = [_P]
    lib.lpf_set_pipelined.argtypes = [_P, ctypes.c_int]
    if hasattr(lib, "lpf_set_geometry"):                     # lab builds only (-DLPF_LAB)
        lib.lpf_set_geometry.argtypes = [_P, ctypes.c_int]
        lib.lpf_lab_role_clock.argtypes = [_P, _P, ctypes.c_int]
        lib.lpf_lab_set_range_limits.argtypes = [_P, ctypes.c_longlong, ctypes.c_int]
        lib.lpf_lab_last_ranges.argtypes = [_P]
    lib.lpf_allreduce_metrics.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, _P]
    lib.lpf_set_camera.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double]
    lib.lpf_set_masks_u8.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.lpf_set_mask_rects.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.lpf_set_masks_rle.argtypes = [_P, ctypes.POINTER(RleMasksInput)]
    lib.lpf_set_masks_ids.argtypes = [_P, ctypes.POINTER(IdMasksInput)]
    lib.lpf_run_wide_ids.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(IdMasksInput), ctypes.POINTER(WideOutputs)]
    lib.lpf_set_erosion_element.argtypes = [_P, ctypes.c_int]
    lib.lpf_resize_masks_u8.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int]
    lib.lpf_erode_masks_u8.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int]
    lib.lpf_set_masks_f32.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.lpf_set_label_image.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.lpf_get_label_image.argtypes = [_P, _P, ctypes.c_int]
    lib.lpf_set_boxes.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int]
    lib.lpf_set_boxes_ex.argtypes = [_P, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int]
    lib.lpf_set_boxes_cam0.argtypes = [_P, _P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P]
    lib.lpf_run.argtypes = [_P, _P, _I64, ctypes.c_int, ctypes.POINTER(Outputs)]
    lib.lpf_run_batch.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(Outputs)]
    lib.lpf_run_frame.argtypes = [_P, ctypes.POINTER(FrameJob)]
    lib.lpf_run_frame_wide.argtypes = [_P, ctypes.POINTER(FrameJobWide)]
    lib.lpf_run_wide.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(WideInput), ctypes.POINTER(WideOutputs)]
    lib.lpf_depth_maps.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(WideInput), ctypes.POINTER(DepthMapsOutputs)]
    lib.lpf_depth_overlays.argtypes = [_P, ctypes.c_int, ctypes.POINTER(DepthOverlayInput), ctypes.POINTER(DepthOverlayOutputs)]
    lib.lpf_match_2d.argtypes = [_P, ctypes.c_int, ctypes.POINTER(Match2dInput), ctypes.POINTER(Match2dOutputs)]
    lib.lpf_assign_costs.argtypes = [_P, ctypes.c_int, ctypes.POINTER(AssignInput), ctypes.POINTER(AssignOutputs)]
    lib.lpf_assign_2d.argtypes = [_P, ctypes.c_int, ctypes.POINTER(Match2dInput), ctypes.POINTER(Assign2dParams), ctypes.POINTER(Assign2dOutputs)]
    lib.lpf_inside_masks.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(InsideInput), ctypes.POINTER(InsideOutputs)]
    lib.lpf_box_points.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(BoxPointsInput), ctypes.POINTER(BoxPointsOutputs)]
    lib.lpf_box_views.argtypes = [_P, ctypes.c_int, ctypes.POINTER(BoxViewsInput), ctypes.POINTER(BoxViewsOutputs)]
    lib.lpf_first_match.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(FirstMatchInput), ctypes.POINTER(FirstMatchOutputs)]
    lib.lpf_depth_maps_rle.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(RleMasksInput), ctypes.POINTER(DepthMapsOutputs)]
    lib.lpf_first_match_rle.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(FirstMatchRleInput),
                                        ctypes.POINTER(FirstMatchOutputs)]
    lib.lpf_run_cams.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(CamInput), ctypes.c_int, ctypes.POINTER(Outputs)]
    lib.lpf_run_cams_wide.argtypes = [_P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(CamInput), ctypes.c_int, ctypes.POINTER(WideOutputs)]
    lib.lpf_points_in_boxes.argtypes = [_P, _P, _I64, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int]
    lib.lpf_depth_image.argtypes = [_P, _P, _I64, ctypes.c_int, _P, _P]
    lib.lpf_prepare_boxes.argtypes = [_P, _P, ctypes.c_int, _P, _P, _P, _P, _P]
    lib.lpf_graph_begin.argtypes = [_P]
    lib.lpf_graph_end.argtypes = [_P, ctypes.POINTER(_P)]
    lib.lpf_graph_launch.argtypes = [_P, _P]
    lib.lpf_graph_destroy.argtypes = [_P]
    lib.lpf_graph_destroy.restype = None
    lib.lpf_get_stats.argtypes = [_P, _P, ctypes.c_int, ctypes.c_int]
    lib.lpf_profile_enable.argtypes = [_P, ctypes.c_int]
    lib.lpf_profile_read.argtypes = [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I64), ctypes.c_int]
    lib.lpf_profile_overhead.argtypes = [_P, ctypes.POINTER(ctypes.c_double)]
    lib.lpf_reader_create.argtypes = [_P, ctypes.POINTER(_P), ctypes.c_int, _I64]
    lib.lpf_reader_submit.argtypes = [_P, ctypes.c_char_p]
    lib.lpf_reader_next.argtypes = [_P, ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.POINTER(_I64)]
    lib.lpf_reader_submit_frame.argtypes = [_P, ctypes.c_char_p, ctypes.c_char_p]
    lib.lpf_reader_boxes.argtypes = [_P, ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.lpf_parse_boxes_json.argtypes = [ctypes.c_char_p, _P, _P, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.lpf_reader_wait.argtypes = [_P]
    lib.lpf_reader_destroy.argtypes = [_P]
    lib.lpf_reader_destroy.restype = None
    _libs[path] = lib
    return lib


EXPORTED = ("lpf_abi_version", "lpf_build_id", "lpf_host_alloc", "lpf_host_free", "lpf_create", "lpf_destroy", "lpf_last_error", "lpf_set_stream", "lpf_use_own_stream", "lpf_wait_for_stream",
            "lpf_release_to_stream", "lpf_sync",
            "lpf_set_pipelined", "lpf_allreduce_metrics",
            "lpf_set_camera", "lpf_set_masks_u8", "lpf_set_masks_f32", "lpf_set_mask_rects", "lpf_set_label_image",
            "lpf_get_label_image", "lpf_set_boxes", "lpf_set_boxes_ex", "lpf_set_boxes_cam0", "lpf_run", "lpf_run_batch", "lpf_run_frame",
            "lpf_points_in_boxes", "lpf_prepare_boxes", "lpf_depth_image", "lpf_resize_masks_u8", "lpf_erode_masks_u8", "lpf_get_stats", "lpf_profile_enable", "lpf_profile_read", "lpf_profile_overhead",
            "lpf_graph_begin", "lpf_graph_end", "lpf_graph_launch", "lpf_graph_destroy",
            "lpf_reader_create", "lpf_reader_submit", "lpf_reader_next", "lpf_reader_wait", "lpf_reader_destroy",
            "lpf_reader_submit_frame", "lpf_reader_boxes", "lpf_parse_boxes_json", "lpf_run_wide", "lpf_run_cams",
            "lpf_run_cams_wide", "lpf_run_frame_wide", "lpf_depth_maps", "lpf_depth_overlays", "lpf_match_2d",
            "lpf_inside_masks", "lpf_set_erosion_element", "lpf_box_points", "lpf_box_views", "lpf_assign_costs", "lpf_assign_2d",
            "lpf_first_match", "lpf_set_masks_rle", "lpf_depth_maps_rle", "lpf_first_match_rle", "lpf_set_masks_ids", "lpf_run_wide_ids")

BOXES_PARSED, BOXES_ABSENT, BOXES_OTHER, BOXES_NONE = 0, 1, 2, 3          # enum lpf_boxes_state


def parse_boxes_file(path):
    """``(state, index int32[B], corners_cam0 f64[B,8,3])`` of a ``BBoxes_<frame>.json`` file, parsed by the library
    (lpf_parse_boxes_json: no GPU involved; the doubles are json.load's).  state: BOXES_PARSED, BOXES_ABSENT (no such file) or
    BOXES_OTHER -- the file is not the plain ``[{"index": int, "corners_cam0": 8 x 3 numbers}, ...]`` and was not interpreted (use
    json.load)."""
    lib = load()
    path = os.fspath(path)
    try:
        cap = os.path.getsize(path) // 64 + 1          # (a box is at least 92 characters of text)
    except OSError:
        cap = 0
    corners, index = np.empty((cap, 8, 3), np.float64), np.empty(cap, np.int32)
    n, st = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.lpf_parse_boxes_json(path.encode(), corners.ctypes.data if cap else None, index.ctypes.data if cap else None, cap,
                                  ctypes.byref(n), ctypes.byref(st))
    if rc != 0:
        raise LpfError(rc, "lpf_parse_boxes_json(%s): %d boxes, room for %d" % (path, n.value, cap))
    if st.value != BOXES_PARSED:
        return st.value, np.empty(0, np.int32), np.empty((0, 8, 3), np.float64)
    return BOXES_PARSED, index[:n.value], corners[:n.value]


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _dev_ptr(t, dtype_name=None):
    """data_ptr of a contiguous torch ROCm tensor (or None)."""
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError("device buffers must be contiguous torch tensors on the GPU")
    if dtype_name is not None and str(t.dtype) != "torch." + dtype_name:
        raise ValueError("expected torch.%s, got %s" % (dtype_name, t.dtype))
    return t.data_ptr()


def _ptr(a):
    """What the library is given for a NumPy array or a contiguous GPU tensor: its address, NULL for None and for an empty one."""
    if a is None:
        return None
    if _is_torch(a):
        return _dev_ptr(a) if a.numel() else None
    return a.ctypes.data if a.size else None


class Scan:
    """One velodyne scan handed out by ScanReader: ``points`` is a float32 [N,4] NumPy view of the
    pinned host copy (what loadVelodyneData returns, V3:24-28), ``dev_ptr`` its copy in HBM.  Both
    are only valid until the reader's next scan is fetched; copy ``points`` to keep it."""
    __slots__ = ("path", "n", "points", "dev_ptr", "_reader", "_ticket", "boxes_state", "box_index", "boxes_cam0")

    def __init__(self, path, n, points, dev_ptr, reader, ticket, boxes_state=BOXES_NONE, box_index=None, boxes_cam0=None):
        self.path, self.n, self.points, self.dev_ptr, self._reader, self._ticket = path, n, points, dev_ptr, reader, ticket
        # the frame's box file when the reader was given one (ScanReader(box_paths=...)): BOXES_* and, when PARSED, COPIES of the
        # reader's arrays: int32 [B], float64 [B,8,3]
        self.boxes_state, self.box_index, self.boxes_cam0 = boxes_state, box_index, boxes_cam0

    def _check_live(self):
        if self._reader._ticket != self._ticket or self._reader._h is None:
            raise LpfError(-3, "this Scan's buffers were recycled (a later scan has been fetched from its reader)")


class ScanReader:
    """Iterator over velodyne .bin files with read-ahead: a native worker thread reads the next files
    into pinned memory and copies them to HBM while the current scan is processed (lpf_reader_*).
    A missing file raises LpfError('<path> does not exist!') for that scan, like V3:26-27."""

    def __init__(self, ctx, paths, n_buffers=3, max_points=1 << 21, box_paths=None):
        self._ctx, self._lib = ctx, ctx._lib
        self._h = None
        self._ticket = 0
        self._paths = [os.fspath(p) for p in paths]
        # box_paths[i]: the BBoxes_<frame>.json of scan i (or None) -- parsed by the reader's worker beside the scan
        self._box_paths = None if box_paths is None else [None if b is None else os.fspath(b) for b in box_paths]
        if self._box_paths is not None and len(self._box_paths) != len(self._paths):
            raise ValueError("box_paths: one entry per scan")
        self._next_submit = 0
        self._delivered = 0
        self._depth = int(n_buffers)
        h = _P()
        ctx._check(self._lib.lpf_reader_create(ctx._h, ctypes.byref(h), int(n_buffers), int(max_points)))
        self._h = h
        ctx._readers.add(self)                  # the context closes its readers before it goes away
        self._top_up()

    def _top_up(self):                         # keep n_buffers - 1 scans ahead of the consumer
        while self._next_submit < len(self._paths) and self._next_submit - self._delivered < self._depth:
            bp = self._box_paths[self._next_submit] if self._box_paths is not None else None
            self._ctx._check(self._lib.lpf_reader_submit_frame(self._h, self._paths[self._next_submit].encode(), bp.encode() if bp else None))
            self._next_submit += 1

    def __iter__(self):
        return self

    def __len__(self):
        return len(self._paths)

    def __next__(self):
        if self._h is None or self._delivered >= len(self._paths):
            raise StopIteration
        path = self._paths[self._delivered]
        d, hp, n = _P(), _P(), _I64(0)
        self._ticket += 1
        rc = self._lib.lpf_reader_next(self._h, ctypes.byref(d), ctypes.byref(hp), ctypes.byref(n))
        self._delivered += 1
        self._top_up()
        self._ctx._check(rc)
        cnt = int(n.value)
        if cnt:
            buf = (ctypes.c_float * (cnt * 4)).from_address(hp.value)
            pts = np.frombuffer(buf, dtype=np.float32).reshape(cnt, 4)
        else:
            pts = np.zeros((0, 4), np.float32)
        state, bidx, bcam = BOXES_NONE, None, None
        if self._box_paths is not None:
            pc, pi, nb, st = _P(), _P(), ctypes.c_int(0), ctypes.c_int(BOXES_NONE)
            self._ctx._check(self._lib.lpf_reader_boxes(self._h, ctypes.byref(pc), ctypes.byref(pi), ctypes.byref(nb), ctypes.byref(st)))
            state = int(st.value)
            if state == BOXES_PARSED:
                b = int(nb.value)
                if b:
                    bcam = np.frombuffer((ctypes.c_double * (b * 24)).from_address(pc.value), dtype=np.float64).reshape(b, 8, 3).copy()
                    bidx = np.frombuffer((ctypes.c_int32 * b).from_address(pi.value), dtype=np.int32).copy()
                else:
                    bcam, bidx = np.empty((0, 8, 3), np.float64), np.empty(0, np.int32)
        return Scan(path, cnt, pts, d.value, self, self._ticket, state, bidx, bcam)

    def wait(self):
        self._ctx._check(self._lib.lpf_reader_wait(self._h))

    def close(self):
        if self._h is not None:
            self._lib.lpf_reader_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LpfContext:
    """One context = one GPU + one stream (not thread-safe): the C ABI, object-shaped."""

    def __init__(self, device=0, library=None):
        self._lib = load(library)
        self.library = dict(self._lib._lpf_info)            # {"path", "build_id"}: which binary, built from which sources
        h = _P()
        rc = self._lib.lpf_create(ctypes.byref(h), int(device))
        if rc != 0:
            raise LpfError(rc, (self._lib.lpf_last_error(None) or b"").decode())
        self._h = h
        self._readers = weakref.WeakSet()
        self.device = int(device)
        self.W = self.H = 0
        self.M = 0
        self.F_masks = 0
        self.box_off = None
        self._depth = 1
        self.erosion_kernel_size = 3            # the element in force (set_erosion_element)
        self._pin = {}                          # persistent page-locked host buffers (run_batch(pinned=True))
        # lent tensors (masks, box corners) of the runs that may still read them: in the pipelined modes a run's inputs are read
        # up to two launches after it was queued, so the references of the last few runs are kept (torch's caching allocator is
        # ordered with torch's stream, not with this context's)
        self._lent = collections.deque(maxlen=4)

    # -- plumbing ---------------------------------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise LpfError(rc, (self._lib.lpf_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            for r in list(getattr(self, "_readers", ())):      # a reader holds pointers into its context
                r.close()
            self._lib.lpf_destroy(self._h)
            self._h = None
            for p, _, _ in self._pin.values():              # (views handed out earlier must not be used after close)
                self._lib.lpf_host_free(p)
            self._pin = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_ptr):
        """Run on the caller's HIP stream, given by its handle (``torch.cuda.current_stream().cuda_stream``; 0 is the
        null stream = torch's default stream).  ``None`` goes back to an internal stream of the context's own."""
        if stream_ptr is None:
            self._check(self._lib.lpf_use_own_stream(self._h))
        else:
            self._check(self._lib.lpf_set_stream(self._h, _P(int(stream_ptr))))

    def wait_for_stream(self, stream_ptr):
        """Device-side edge: the context's stream(s) wait for everything queued so far on ``stream_ptr`` (a HIP stream
        handle, 0 = the null stream).  Needed when the context runs on its own stream and the inputs -- or the memory of
        the output tensors -- were last touched on another stream."""
        self._check(self._lib.lpf_wait_for_stream(self._h, _P(int(stream_ptr))))

    def release_to_stream(self, stream_ptr):
        """Device-side edge the other way: ``stream_ptr`` waits for everything this context has queued."""
        self._check(self._lib.lpf_release_to_stream(self._h, _P(int(stream_ptr))))

    def _call_in_order(self, device, fn, *args):
        """One native call ``fn(handle, *args)``.  device None (host arrays): plainly.  A torch device (GPU tensors): in torch's stream
        order (include/lpf.h, "Ordering contract") -- the inputs, and the memory torch's caching allocator handed out for the outputs,
        belong to torch's current stream, the kernels run on the context's: an edge in, an edge out (no-ops when the two are one)."""
        if device is None:
            self._check(fn(self._h, *args))
            return
        import torch
        ts = torch.cuda.current_stream(device).cuda_stream
        self.wait_for_stream(ts)
        self._check(fn(self._h, *args))
        self.release_to_stream(ts)

    def sync(self):
        self._check(self._lib.lpf_sync(self._h))
        self._lent.clear()

    PIPELINED = {False: 0, 0: 0, None: 0, "off": 0, "fused": 2, 2: 2, "fused-pack": 4, 4: 4}

    def set_pipelined(self, on="fused-pack"):
        """Software-pipelined device-mode runs (lpf_set_pipelined).  ``"fused"``: the tail of a run rides in the next run's
        launch (one launch per run).  ``"fused-pack"``: the packing of lent uint8 masks rides too -- the launch of a run carries
        its mask pack, the streaming work of the run before, the tail of the one before that; a run's points and outputs are in
        use until the launch after the next.  ``False`` switches it off.  Results of a run are complete after sync() /
        release_to_stream().  Masks are set before every run; boxes set for a run travel with it (no drain)."""
        if on is True:
            raise ValueError('set_pipelined(True) meant the stream-pipelined modes 1 / 3, removed in ABI 5: use "fused" or "fused-pack"')
        if on not in self.PIPELINED:
            raise ValueError('set_pipelined: False, "fused" or "fused-pack"')
        self._check(self._lib.lpf_set_pipelined(self._h, self.PIPELINED[on]))
        self._depth = 3 if self.PIPELINED[on] else 1
        self._lent = collections.deque(self._lent, maxlen=2 * self._depth + 2)

    def set_geometry(self, mode="auto"):
        """LAB BUILDS ONLY (LPF_LIBRARY=liblpf_lab.so).  Segment / tile sizes of a run: "auto" (by launch size, what the product
        does), "small" (1024-point segments, wide tail), "small-narrow", "large" (4096) or "large-scan" (4096, prefixes from
        the scan kernel); same results."""
        if not hasattr(self._lib, "lpf_set_geometry"):
            raise LpfError(-3, "lpf_set_geometry exists in lab builds only (python -m lidar_object_detection_amd._build lab; LPF_LIBRARY=...)")
        self._check(self._lib.lpf_set_geometry(self._h, {"auto": 0, "small": 1, "large": 2, "large-scan": 3, "small-narrow": 4, "small-1024": 5}[mode]))

    def set_range_limits(self, budget=0, max_items=0):
        """LAB BUILDS ONLY.  Range limits of the batched analysis calls (match_2d, assign_costs, assign_2d, inside_masks, box_points,
        box_views, first_match, depth_maps, depth_overlays): budget = the staging bytes of a range, max_items = the most frames / images
        of a range or launch (never above the product's limit); 0 = the product's value.  Same results."""
        if not hasattr(self._lib, "lpf_lab_set_range_limits"):
            raise LpfError(-3, "lpf_lab_set_range_limits exists in lab builds only (python -m lidar_object_detection_amd._build lab; LPF_LIBRARY=...)")
        self._check(self._lib.lpf_lab_set_range_limits(self._h, int(budget), int(max_items)))

    def last_ranges(self):
        """LAB BUILDS ONLY.  The ranges (chunks) the last batched analysis call planned; for inside_masks and box_points the launches
        of their frame loop."""
        if not hasattr(self._lib, "lpf_lab_last_ranges"):
            raise LpfError(-3, "lpf_lab_last_ranges exists in lab builds only (python -m lidar_object_detection_amd._build lab; LPF_LIBRARY=...)")
        return int(self._lib.lpf_lab_last_ranges(self._h))

    ROLES = ("summaries", "box job", "lists", "box counts", "mask pack", "project+label tiles")

    def role_clock(self, reset=True):
        """LAB BUILDS ONLY.  Per role of the step launches of the software-pipelined modes since the last reset: {role: dict(span_us =
        first block start .. last block end, blocks, mean_us, longest_us)}; the first call switches the clock on.  Synchronises."""
        if not hasattr(self._lib, "lpf_lab_role_clock"):
            raise LpfError(-3, "lpf_lab_role_clock exists in lab builds only (python -m lidar_object_detection_amd._build lab; LPF_LIBRARY=...)")
        a = np.zeros((6, 5), np.uint64)
        self._check(self._lib.lpf_lab_role_clock(self._h, a.ctypes.data, 1 if reset else 0))
        out = {}
        for r, name in enumerate(self.ROLES):
            n = int(a[r, 3])
            if n:
                out[name] = dict(span_us=(int(a[r, 1]) - int(a[r, 0])) / 100.0, blocks=n, mean_us=int(a[r, 2]) / 100.0 / n, longest_us=int(a[r, 4]) / 100.0,
                                 first_start_tick=int(a[r, 0]), last_end_tick=int(a[r, 1]))
        return out

    def allreduce_metrics(self, vec, rccl_comm, op="sum"):
        """In-place all-reduce of an int64 NumPy vector over an RCCL communicator (an ncclComm_t as an integer /
        c_void_p, e.g. from ncclCommInitRank through ctypes); op: "sum", "min" or "max"."""
        a = np.ascontiguousarray(vec, dtype=np.int64)
        self._check(self._lib.lpf_allreduce_metrics(self._h, a.ctypes.data, int(a.size), {"sum": 0, "min": 1, "max": 2}[op],
                                                    rccl_comm if isinstance(rccl_comm, ctypes.c_void_p) else _P(rccl_comm)))
        return a

    def graph_begin(self):
        """Start capturing the device-mode calls made on this context into a hipGraph."""
        self._check(self._lib.lpf_graph_begin(self._h))

    def graph_end(self):
        """Finish the capture; returns an opaque handle for graph_launch()."""
        g = _P()
        self._check(self._lib.lpf_graph_end(self._h, ctypes.byref(g)))
        return g

    def graph_launch(self, g):
        self._check(self._lib.lpf_graph_launch(self._h, g))

    def graph_destroy(self, g):
        self._lib.lpf_graph_destroy(g)

    STATS = ("host_waits", "drains", "uploads", "step_launches", "box_jobs_alone", "box_jobs_riding", "blocking_uploads",
             "wide_direct_frames")

    def stats(self, reset=False):
        """dict of lpf_get_stats: what the context has done so far (host waits, drains, uploads, launches)."""
        a = np.zeros(8, np.int64)
        self._check(self._lib.lpf_get_stats(self._h, a.ctypes.data, 8, int(bool(reset))))
        return dict(zip(self.STATS, (int(v) for v in a)))

    def profile_enable(self, on=True):
        self._check(self._lib.lpf_profile_enable(self._h, int(bool(on))))

    def profile_read(self, reset=True):
        """(summed milliseconds, launches) of the event-bracketed project+label kernel."""
        ms, n = ctypes.c_double(0.0), _I64(0)
        self._check(self._lib.lpf_profile_read(self._h, ctypes.byref(ms), ctypes.byref(n), int(bool(reset))))
        return ms.value, int(n.value)

    def profile_overhead(self):
        """Milliseconds between two event records with nothing in between (what a bracket adds to a kernel)."""
        ms = ctypes.c_double(0.0)
        self._check(self._lib.lpf_profile_overhead(self._h, ctypes.byref(ms)))
        return ms.value

    # -- state ------------------------------------------------------------------------
    def set_camera(self, T_velo_to_rect, K, width, height, depth_min=0.0, depth_max=50.0):
        T = np.ascontiguousarray(T_velo_to_rect, dtype=np.float64).reshape(16)
        K3 = np.ascontiguousarray(np.asarray(K, dtype=np.float64)[:3, :3]).reshape(9)
        key = (T.tobytes(), K3.tobytes(), int(width), int(height), float(depth_min), float(depth_max))
        if key == getattr(self, "_camera", None):           # a frame loop sets the same camera every frame: nothing to do (the C call
            return                                          # would mark captured graphs stale and wait for work still owed)
        self._check(self._lib.lpf_set_camera(self._h, T.ctypes.data, K3.ctypes.data, int(width), int(height),
                                             float(depth_min), float(depth_max)))
        self._camera = key
        self.W, self.H = int(width), int(height)

    def ensure_intrinsics(self, K, width, height):
        """The camera's K, width and height are in force -- all that lpf_prepare_boxes reads of the camera.  A frame loop that prepares
        boxes and runs frames in turn keeps the run's camera (no lpf_set_camera per frame: that call waits for work still owed)."""
        K3 = np.ascontiguousarray(np.asarray(K, dtype=np.float64)[:3, :3]).reshape(9)
        cam = getattr(self, "_camera", None)
        if cam is not None and cam[1] == K3.tobytes() and cam[2] == int(width) and cam[3] == int(height):
            return
        self.set_camera(np.eye(4), K3.reshape(3, 3), width, height, 0.0, 1.0)

    BINARIZE = {"astype": 0, "v3": 1, "gt0.5": 2}

    def resize_masks(self, masks):
        """cv2.resize(mask.astype(np.uint8), (W, H)) (V3:222, INTER_LINEAR) for masks [..., h, w] that are not at the camera's size:
        returns uint8 [..., H, W] -- a NumPy array for a NumPy / list input, a torch GPU tensor for a uint8 torch GPU tensor (in stream
        order).  Float masks are cast first, as the reference casts them (``astype(np.uint8)``: truncation).  Restated from OpenCV's
        C++ reference path, pinned by construction only (oracle/numpy_path.py: cv2_resize_linear_u8)."""
        if _is_torch(masks):
            import torch
            if str(masks.dtype) != "torch.uint8" or not masks.is_contiguous():
                masks = masks.to(torch.uint8).contiguous()       # (torch's float -> uint8 cast truncates, as astype does for 0 <= v < 256)
            shape = tuple(masks.shape)
            out = torch.empty(shape[:-2] + (self.H, self.W), dtype=torch.uint8, device=masks.device)
            n = int(np.prod(shape[:-2], dtype=np.int64)) if len(shape) > 2 else 1
            self._call_in_order(masks.device, self._lib.lpf_resize_masks_u8, _dev_ptr(masks) if n else None, n, shape[-2], shape[-1],
                                _dev_ptr(out) if n else None, 1)           # the caller may use `out` on torch's stream at once
            return out
        a = np.asarray(masks)
        a = np.ascontiguousarray(a.astype(np.uint8))
        shape = a.shape
        out = np.empty(shape[:-2] + (self.H, self.W), np.uint8)
        n = int(np.prod(shape[:-2], dtype=np.int64)) if len(shape) > 2 else 1
        self._check(self._lib.lpf_resize_masks_u8(self._h, a.ctypes.data if n else None, n, shape[-2], shape[-1], out.ctypes.data if n else None, 0))
        return out

    def set_erosion_element(self, k):
        """The element of every erosion this context performs from now on: cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (k, k)), the
        reference's ``erosion_kernel_size`` (V3:55-97; include/lpf.h: lpf_set_erosion_element) -- k odd, 1 .. 15, 3 (the cross) in a
        new context.  It holds for set_masks' / run_wide's / run_cams' / depth_maps' ``erode_iters`` and for erode_masks; masks that are
        packed already keep theirs.  Host state only: nothing is queued.  A refused size raises LpfError and changes nothing."""
        self._check(self._lib.lpf_set_erosion_element(self._h, int(k)))
        self.erosion_kernel_size = int(k)

    def erode_masks(self, masks, iterations=1):
        """cv2.erode(plane, MORPH_ELLIPSE k x k, iterations) on uint8 VALUES [..., h, w] at the planes' own size (V3:83-90, for masks that
        are eroded before they are resized), k = the context's element (set_erosion_element; 3 by default): NumPy in -> NumPy out,
        uint8 torch GPU tensor in -> tensor out (ordered with torch's current stream on both sides)."""
        if _is_torch(masks):
            import torch
            if str(masks.dtype) != "torch.uint8" or not masks.is_contiguous():
                raise ValueError("device masks must be a contiguous uint8 tensor")
            shape = tuple(masks.shape)
            out = torch.empty_like(masks)
            n = int(np.prod(shape[:-2], dtype=np.int64)) if len(shape) > 2 else 1
            self._call_in_order(masks.device, self._lib.lpf_erode_masks_u8, _dev_ptr(masks) if n else None, n, shape[-2], shape[-1],
                                int(iterations), _dev_ptr(out) if n else None, 1)
            return out
        a = np.ascontiguousarray(np.asarray(masks), dtype=np.uint8)
        out = np.empty_like(a)
        n = int(np.prod(a.shape[:-2], dtype=np.int64)) if a.ndim > 2 else 1
        self._check(self._lib.lpf_erode_masks_u8(self._h, a.ctypes.data if n else None, n, a.shape[-2], a.shape[-1], int(iterations), out.ctypes.data if n else None, 0))
        return out

    def set_mask_rects(self, rects):
        """Hint for the NEXT set_masks call: rects int32 [M,4] or [F,M,4] = (x0, y0, x1, y1), half open, pixels -- mask m of frame f is
        zero outside its rectangle (a detector's masks come cropped to their 2D boxes).  Where uint8 masks are packed as they are the
        pack then only reads what lies inside; anything else ignores the hint; results do not change as long as the word holds.  NumPy
        array (copied now) or an int32 torch GPU tensor (read when the masks are packed: keep it unchanged until then).  None clears."""
        if rects is None:
            self._check(self._lib.lpf_set_mask_rects(self._h, None, 0, 0, 0))
            return
        dev = _is_torch(rects)
        shape = tuple(rects.shape)
        if len(shape) == 2:
            shape = (1,) + shape
        if len(shape) != 3 or shape[2] != 4:
            raise ValueError("rects must be [M,4] or [F,M,4], got %s" % (shape,))
        if dev:
            if str(rects.dtype) != "torch.int32" or not rects.is_contiguous():
                raise ValueError("device rects must be a contiguous int32 tensor")
            self._lent.append(rects)
            self._check(self._lib.lpf_set_mask_rects(self._h, _dev_ptr(rects), 1, shape[0], shape[1]))
        else:
            a = np.ascontiguousarray(rects, dtype=np.int32)
            self._check(self._lib.lpf_set_mask_rects(self._h, a.ctypes.data, 0, shape[0], shape[1]))

    @staticmethod
    def mask_rects(masks):
        """Tight rectangles [..., M, 4] (x0, y0, x1, y1; half open; an empty mask gets 0, 0, 0, 0) of host masks [..., M, H, W]: what a
        detector's 2D boxes give for masks cropped to them."""
        m = np.asarray(masks) != 0
        ys, xs = m.any(axis=-1), m.any(axis=-2)
        def span(b):
            any_ = b.any(axis=-1)
            lo = np.where(any_, b.argmax(axis=-1), 0)
            hi = np.where(any_, b.shape[-1] - b[..., ::-1].argmax(axis=-1), 0)
            return lo, hi
        y0, y1 = span(ys)
        x0, x1 = span(xs)
        return np.stack([x0, y0, x1, y1], axis=-1).astype(np.int32)

    def set_masks(self, masks, erode_iters=0, v3_pipeline=False, binarize=None, lend=False):
        """masks: [M,H,W] or [F,M,H,W]; uint8/bool (nonzero = member) or float32 (reference masks).
        NumPy array, or torch tensor already on the GPU.  Float masks: ``binarize`` is "astype"
        (mask.astype(uint8) != 0, V3:222-225), "v3" (the V3:82-97 erosion block's casts; same as
        v3_pipeline=True) or "gt0.5" (mask > 0.5, Same_color.py:125 / vis.py:185).
        lend=True (GPU tensors): the tensor stays untouched until the runs that use these masks have completed, so a
        small launch may read it directly instead of packing it first, and in the "fused-pack" mode its pack rides in the
        run's launch (on_device = 2 of the C ABI).  The context keeps references to the lent tensors of the last few runs
        (until sync() at the latest); the CALLER must not rewrite a lent tensor before the run's results are complete."""
        if binarize is None:
            binarize = "v3" if v3_pipeline else "astype"
        if binarize not in self.BINARIZE:
            raise ValueError("binarize must be one of %s" % sorted(self.BINARIZE))
        dev = _is_torch(masks)
        shape = tuple(masks.shape)
        if len(shape) == 3:
            shape = (1,) + shape
        if len(shape) != 4 or (shape[1] and shape[2:] != (self.H, self.W)):
            raise ValueError("masks must be [M,%d,%d] or [F,M,%d,%d], got %s" % (self.H, self.W, self.H, self.W, shape))
        F, M = shape[0], shape[1]
        if dev:
            is_f = str(masks.dtype) == "torch.float32"
            if not is_f and str(masks.dtype) not in ("torch.uint8", "torch.bool"):
                raise ValueError("device masks must be float32, uint8 or bool")
            ptr = _dev_ptr(masks) if M else None
            keep = masks
        else:
            a = np.asarray(masks)
            is_f = a.dtype.kind == "f"
            a = np.ascontiguousarray(a, dtype=np.float32 if is_f else np.uint8)
            ptr = a.ctypes.data if M else None
            keep = a
        where = (2 if lend else 1) if dev else 0
        if is_f:
            rc = self._lib.lpf_set_masks_f32(self._h, ptr, F, M, self.BINARIZE[binarize], int(erode_iters), where)
        else:
            rc = self._lib.lpf_set_masks_u8(self._h, ptr, F, M, int(erode_iters), where)
        if dev and lend:
            self._lent.append(keep)
        del keep
        self._check(rc)
        self.F_masks, self.M = F, M

    @staticmethod
    def rle_batch(frames_masks, H, W, max_masks=LPF_MAX_MASKS, who="set_masks_rle"):
        """``(runs int32 [Rtot,2], run_off int64 [F*M + 1], F, M)`` of one RleMasks or a list of them, one per frame, as lpf_set_masks_rle
        -- or a pass that takes up to ``max_masks`` run-length masks per frame (run_wide, run_cams, run_cams_wide) -- takes them: frames
        with fewer masks than the largest are padded with empty masks.  ValueError -- before any native call, with ``who`` as the
        message's prefix -- for anything that is not an RleMasks, a size other than H x W, more than max_masks masks, and runs of another
        dtype or shape or out of bounds (they are checked again here: the fields of an RleMasks can be assigned)."""
        from .rle import check_runs
        frames = [frames_masks] if isinstance(frames_masks, RleMasks) else list(frames_masks)
        for f, r in enumerate(frames):
            if not isinstance(r, RleMasks):
                raise ValueError("%s: frame %d is %s, not RleMasks" % (who, f, type(r).__name__))
            if tuple(r.shape[1:]) != (H, W):
                raise ValueError("%s: frame %d has masks of %d x %d, the camera is %d x %d (runs are not resized)"
                                 % (who, f, r.shape[2], r.shape[1], W, H))
            if r.shape[0] > max_masks:
                raise ValueError("%s: frame %d has %d masks, one pass takes %d (pipeline.run_frames groups them)"
                                 % (who, f, r.shape[0], max_masks))
        F = len(frames)
        M = max([r.shape[0] for r in frames], default=0)
        checked = [check_runs(r.runs, r.run_off, r.shape[0], H * W, "%s: frame %d" % (who, f)) for f, r in enumerate(frames)]
        run_off = np.zeros(F * M + 1, np.int64)
        base = 0
        for f, (runs, off) in enumerate(checked):
            m = len(off) - 1
            run_off[f * M + 1:f * M + 1 + m] = base + off[1:]
            base += len(runs)
            run_off[f * M + 1 + m:(f + 1) * M + 1] = base
        runs = np.concatenate([c[0] for c in checked]) if checked else np.zeros((0, 2), np.int32)
        return np.ascontiguousarray(runs, dtype=np.int32), run_off, F, M

    def set_masks_rle(self, frames_masks, erode_iters=0):
        """Masks in run-length form (rle.RleMasks: one, or a list with one per frame), decoded on the GPU: what reaches the device is
        the runs -- a few tens of KB for a frame's masks -- instead of M x H x W bytes.  Afterwards the context is as after
        ``set_masks(dense uint8 host masks, erode_iters)`` with the same members.  Ragged M is padded with empty masks; the masks must
        have the camera's size; at most LPF_MAX_MASKS per frame (pipeline.run_frames groups more)."""
        runs, run_off, F, M = self.rle_batch(frames_masks, self.H, self.W)
        if int(erode_iters) < 0:                            # (not _check_erode_iters: this call has always taken 1.5 as 1, and words it so)
            raise ValueError("erode_iters must be >= 0, got %r" % (erode_iters,))
        inp = RleMasksInput.of(runs, run_off, F, M, erode_iters)
        self._check(self._lib.lpf_set_masks_rle(self._h, ctypes.byref(inp)))
        self.F_masks, self.M = F, M

    def set_masks_ids(self, frames_masks, erode_iters=0):
        """Masks as instance-ID maps (idmap.IdMasks: one, or a list with one per frame), decoded on the GPU: what reaches the device is
        the map -- H * W * 2 or 4 bytes per frame whatever M is -- or nothing when the map is a GPU tensor.  Afterwards the context is
        as after ``set_masks(dense uint8 host masks, erode_iters)`` with the same members.  Ragged M is padded with LPF_ID_NONE; the
        maps must have the camera's size and one dtype; host maps are stacked into one [F,H,W] array, GPU maps must be the frames of one
        contiguous [F,H,W] tensor (or F = 1) and are read where they are; at most LPF_MAX_MASKS per frame (pipeline.run_frames groups
        more)."""
        if compact_frames(frames_masks, "set_masks_ids", ("ids",)) is None and \
                not (isinstance(frames_masks, (list, tuple)) and not len(frames_masks)):
            raise ValueError("set_masks_ids: masks must be an IdMasks or a list of them, got %s" % type(frames_masks).__name__)
        _check_erode_iters(erode_iters)
        maps, sel, F, M, id_bytes, dev = ids_batch(frames_masks, self.H, self.W)
        if dev:
            import torch
            self.wait_for_stream(torch.cuda.current_stream(maps[0].device).cuda_stream)     # the maps were produced on torch's stream
        inp = _ids_input(maps, sel, F, M, id_bytes, dev, erode_iters)
        rc = self._lib.lpf_set_masks_ids(self._h, ctypes.byref(inp))
        if dev:
            self._lent.append(maps)                          # (the decode reads them in stream order)
        self._check(rc)
        self.F_masks, self.M = F, M

    def clear_masks(self):
        self._check(self._lib.lpf_set_masks_u8(self._h, None, 0, 0, 0, 0))
        self.F_masks, self.M = 0, 0

    def set_label_image(self, label, M):
        a = np.ascontiguousarray(label, dtype=np.uint32)
        if a.ndim == 2:
            a = a[None]
        if a.shape[1:] != (self.H, self.W):
            raise ValueError("label image must be [F,%d,%d]" % (self.H, self.W))
        self._check(self._lib.lpf_set_label_image(self._h, a.ctypes.data, a.shape[0], int(M), 0))
        self.F_masks, self.M = a.shape[0], int(M)

    def get_label_image(self):
        out = np.empty((self.F_masks, self.H, self.W), np.uint32)
        self._check(self._lib.lpf_get_label_image(self._h, out.ctypes.data, 0))
        return out

    def set_boxes(self, corners_per_frame, oriented=True):
        """corners_per_frame: list (one entry per frame) of f64 [B_f,8,3] velodyne-frame corners,
        or a single [B,8,3] array for a one-frame run."""
        if isinstance(corners_per_frame, np.ndarray):
            corners_per_frame = [corners_per_frame]
        arrs = [np.asarray(c, dtype=np.float64).reshape(-1, 8, 3) for c in corners_per_frame]
        off = np.zeros(len(arrs) + 1, np.int32)
        off[1:] = np.cumsum([a.shape[0] for a in arrs])
        cat = np.ascontiguousarray(np.concatenate(arrs, axis=0)) if arrs else np.zeros((0, 8, 3))
        self._check(self._lib.lpf_set_boxes(self._h, cat.ctypes.data if cat.size else None, off.ctypes.data,
                                            len(arrs), int(bool(oriented))))
        self.box_off = off

    def set_boxes_device(self, corners, box_off, oriented=True, lend=False):
        """Boxes from a torch float64 GPU tensor [Btot,8,3] (velodyne frame); box_off: host int32 [F+1].  No copy through the
        host and no wait (usable inside graph_begin/end with unchanged box counts).  lend=True: the tensor is read when the
        tables are built -- by the next run's launch in the pipelined modes -- and must stay unchanged until then."""
        off = np.ascontiguousarray(box_off, dtype=np.int32)
        self._check(self._lib.lpf_set_boxes_ex(self._h, _dev_ptr(corners, "float64") if int(off[-1]) else None, 2 if lend else 1, off.ctypes.data,
                                               off.shape[0] - 1, int(bool(oriented))))
        if lend:
            self._lent.append(corners)
        self.box_off = off

    def set_boxes_cam0_device(self, corners_cam0, box_off, T_cam_to_velo, filter_visible=True, oriented=True, lend=False,
                              visible=None, corners_velo=None, bbox2d=None, front=None):
        """set_boxes_cam0 with the cam-0 corners in a torch float64 GPU tensor [Btot,8,3] (and optional GPU output tensors:
        visible uint8 [Btot], corners_velo float64 [Btot,8,3], bbox2d float64 [Btot,4], front int32 [Btot]).  The reference's
        per-frame box preparation (V3:556-562) entirely on the device, without a wait; in the pipelined modes it rides in the
        next run's launch.  lend as in set_boxes_device."""
        off = np.ascontiguousarray(box_off, dtype=np.int32)
        T = np.ascontiguousarray(T_cam_to_velo, dtype=np.float64).reshape(16)
        self._check(self._lib.lpf_set_boxes_cam0(self._h, _dev_ptr(corners_cam0, "float64") if int(off[-1]) else None, 2 if lend else 1,
                                                 off.ctypes.data, off.shape[0] - 1, T.ctypes.data, int(bool(filter_visible)), int(bool(oriented)),
                                                 _dev_ptr(visible, "uint8"), _dev_ptr(corners_velo, "float64"), _dev_ptr(bbox2d, "float64"),
                                                 _dev_ptr(front, "int32")))
        if lend:
            self._lent.append(corners_cam0)
        self.box_off = off

    def set_boxes_cam0(self, corners_cam0_per_frame, T_cam_to_velo, filter_visible=True, oriented=True, want_outputs=True):
        """The reference's per-frame box preparation (filter_visible_bboxes + transform_bboxes_to_velodyne, V3:556-562) and
        set_boxes in one device-side step.  corners_cam0_per_frame: list of f64 [B_f,8,3] (or one array).  Box indices of later
        results refer to the GIVEN boxes; dropped ones have zero counts.  Returns per frame (visible bool[B_f], corners_velo
        [B_f,8,3], bbox2d [B_f,4], front int32[B_f]) unless want_outputs is False."""
        if isinstance(corners_cam0_per_frame, np.ndarray):
            corners_cam0_per_frame = [corners_cam0_per_frame]
        arrs = [np.asarray(c, dtype=np.float64).reshape(-1, 8, 3) for c in corners_cam0_per_frame]
        off = np.zeros(len(arrs) + 1, np.int32)
        off[1:] = np.cumsum([a.shape[0] for a in arrs])
        cat = np.ascontiguousarray(np.concatenate(arrs, axis=0)) if arrs else np.zeros((0, 8, 3))
        T = np.ascontiguousarray(T_cam_to_velo, dtype=np.float64).reshape(16)
        B = int(off[-1])
        vis, cv = np.zeros(B, np.uint8), np.zeros((B, 8, 3), np.float64)
        bb, fr = np.zeros((B, 4), np.float64), np.zeros(B, np.int32)
        w = want_outputs and B > 0
        self._check(self._lib.lpf_set_boxes_cam0(self._h, cat.ctypes.data if B else None, 0, off.ctypes.data, len(arrs), T.ctypes.data,
                                                 int(bool(filter_visible)), int(bool(oriented)), vis.ctypes.data if w else None,
                                                 cv.ctypes.data if w else None, bb.ctypes.data if w else None, fr.ctypes.data if w else None))
        self.box_off = off
        if not want_outputs:
            return None
        return [(vis[a:b].astype(bool), cv[a:b], bb[a:b], fr[a:b]) for a, b in zip(off[:-1], off[1:])]

    def clear_boxes(self):
        self._check(self._lib.lpf_set_boxes(self._h, None, None, 0, 1))
        self.box_off = None

    def points_in_boxes(self, points, corners, oriented=True):
        """bool [B,k]: row b is the reference's oriented_point_in_bbox(points, corners[b]) (or point_in_bbox)."""
        p = np.ascontiguousarray(points, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] not in (3, 4):
            raise ValueError("points must be [k,3] or [k,4]")
        c = np.ascontiguousarray(corners, dtype=np.float64).reshape(-1, 8, 3)
        k, B = p.shape[0], c.shape[0]
        out = np.zeros((B, k), np.uint8)
        if k and B:
            self._check(self._lib.lpf_points_in_boxes(self._h, p.ctypes.data, k, p.shape[1], c.ctypes.data, B,
                                                      int(bool(oriented)), out.ctypes.data, 0))
        return out.astype(bool)

    def depth_image(self, points):
        """(D f64[H,W], winner int32[H,W]) of f32[N,4] host points: depth of the last valid point per pixel."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 4)
        D, win = np.empty((self.H, self.W), np.float64), np.empty((self.H, self.W), np.int32)
        self._check(self._lib.lpf_depth_image(self._h, p.ctypes.data if len(p) else None, p.shape[0], 0,
                                              D.ctypes.data, win.ctypes.data))
        return D, win

    def prepare_boxes(self, corners_cam0, T_cam_to_velo):
        """(visible bool[B], corners_velo f64[B,8,3], bbox2d f64[B,4], front int32[B]) of B annotated boxes
        given by their cam-0 corners: filter_visible_bboxes + transform_bboxes_to_velodyne + V4's projected
        2D box, computed on the GPU with the reference's arithmetic (needs set_camera first)."""
        c = np.ascontiguousarray(corners_cam0, dtype=np.float64).reshape(-1, 8, 3)
        T = np.ascontiguousarray(T_cam_to_velo, dtype=np.float64).reshape(16)
        B = c.shape[0]
        vis, cv = np.zeros(B, np.uint8), np.zeros((B, 8, 3), np.float64)
        bb, fr = np.zeros((B, 4), np.float64), np.zeros(B, np.int32)
        if B:
            self._check(self._lib.lpf_prepare_boxes(self._h, c.ctypes.data, B, T.ctypes.data, vis.ctypes.data, cv.ctypes.data,
                                                    bb.ctypes.data, fr.ctypes.data))
        return vis.astype(bool), cv, bb, fr

    # -- the hot path, host arrays ------------------------------------------------------
    def run(self, points, **kw):
        """One frame of f32[N,4] host points -> dict of NumPy results (see run_batch)."""
        return self.run_batch([points], **kw)[0]

    def _pinned(self, name, shape, dtype):
        """A persistent page-locked host array of the context (grow-only; lpf_host_alloc = hipHostMalloc, no torch involved): copies
        from the GPU into it are DMA transfers the call does not stage through pageable memory, and a frame loop does not allocate
        (and page in) megabytes per call."""
        need = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ent = self._pin.get(name)
        if ent is None or ent[1] < need:
            if ent is not None:
                self._lib.lpf_host_free(ent[0])
                del self._pin[name]
            cap = max(need + need // 4, 4096)
            p = self._lib.lpf_host_alloc(cap)
            if not p:
                raise LpfError(-4, (self._lib.lpf_last_error(None) or b"lpf_host_alloc failed").decode())
            ent = self._pin[name] = (p, cap, np.frombuffer((ctypes.c_uint8 * cap).from_address(p), dtype=np.uint8))
        return ent[2][:need].view(dtype).reshape(shape)

    def _stage_points(self, frames):
        """Where the library reads a run's points: (frame offsets int64 [F+1], pointer, on_device, what must stay alive until the run
        returns).  ONE Scan of a ScanReader is read where it already is, in HBM; ONE float32 [N,4] GPU tensor too (ordered with
        torch's current stream).  Several frames -- host arrays, Scans, GPU tensors -- each go to their place in ONE device tensor:
        no concatenation of the batch on the host first (20 real frames are 37 MB: the copy cost as much as their kernels a hundred
        times over).  Without torch's GPU support they are concatenated on the host."""
        pts = []
        for p in frames:
            if isinstance(p, Scan):
                p._check_live()
            elif _is_torch(p):
                if p.ndim != 2 or p.shape[1] != 4:
                    raise ValueError("device points must be a float32 tensor [N,4]")
            else:
                p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1, 4)
            pts.append(p)
        if not pts:
            raise ValueError("no frames")
        off = np.zeros(len(pts) + 1, np.int64)
        off[1:] = np.cumsum([len(p.points) if isinstance(p, Scan) else int(p.shape[0]) for p in pts])
        n = int(off[-1])
        one = pts[0] if len(pts) == 1 else None
        if isinstance(one, Scan):
            return off, (one.dev_ptr if n else None), 1, one
        if _is_torch(one):
            import torch
            self.wait_for_stream(torch.cuda.current_stream(one.device).cuda_stream)      # the tensor was produced on torch's stream
            return off, (_dev_ptr(one, "float32") if n else None), 1, one
        pts = [p.points if isinstance(p, Scan) else p for p in pts]
        if len(pts) > 1 and n:
            try:
                import torch
                if torch.cuda.is_available():
                    batch = torch.empty((n, 4), dtype=torch.float32, device=torch.device("cuda", self.device))
                    for f, p in enumerate(pts):
                        if p.shape[0]:
                            batch[int(off[f]):int(off[f + 1])].copy_(p if _is_torch(p) else torch.from_numpy(p))
                    self.wait_for_stream(torch.cuda.current_stream(batch.device).cuda_stream)
                    return off, batch.data_ptr(), 1, batch
            except ImportError:
                pass
        host = np.concatenate([p.cpu().numpy() if _is_torch(p) else p for p in pts], axis=0) if len(pts) > 1 else pts[0]
        return off, (host.ctypes.data if n else None), 0, host

    @staticmethod
    def _until_lists_fit(launch, inst_cap, off):
        """launch(inst_cap) -> (outputs, 0 or the capacity the instance lists need when they did not fit): run again with the exact
        capacity, once it is known"""
        o = off.tolist()
        cap = max(max(b - a for a, b in zip(o, o[1:])), 1) if inst_cap is None else inst_cap
        while True:
            out, need = launch(cap)
            if not need:
                return out
            cap = need

    _BOXES_IN_FORCE = object()

    def _frame_results(self, off, M, summ, per_point, per_valid, iidx, cmb, box_off=_BOXES_IN_FORCE):
        """One dict per frame of a run's outputs: the frame's row of the summary columns ``summ`` (n_valid, n_labelled, inst_count,
        inst_off, best_box, best_cnt), its rows of the ``per_point`` arrays [Ntot, ...], the first n_valid rows of its part of the
        ``per_valid`` arrays, its instance lists out of ``iidx`` and its [M, B_f] block of the counts ``cmb`` (boxes: the ones in
        force, or the run's own ``box_off``)."""
        if box_off is self._BOXES_IN_FORCE:
            box_off = self.box_off
        nv, nl, ic, io, bb, bc = (summ[k] for k in ("n_valid", "n_labelled", "inst_count", "inst_off", "best_box", "best_cnt"))
        res = []
        for f in range(len(off) - 1):
            a, b = int(off[f]), int(off[f + 1])
            n_valid = int(nv[f])
            r = dict(n_valid=n_valid, n_labelled=int(nl[f]), inst_count=ic[f, :M].copy(), best_box=bb[f, :M].copy(),
                     best_cnt=bc[f, :M].copy())
            for k, x in per_point.items():
                r[k] = x[a:b]
            for k, x in per_valid.items():
                r[k] = x[a:a + n_valid]
            if per_valid:                                                     # (want_lists)
                o = io[f].tolist()
                r["inst_lists"] = [iidx[f, o[m]:o[m + 1]] for m in range(M)] if iidx is not None else []
            if box_off is not None:
                b0, b1 = int(box_off[f]), int(box_off[f + 1])
                r["count_mb"] = cmb[M * b0:M * b1].reshape(M, b1 - b0).astype(np.int64)
            else:
                r["count_mb"] = np.zeros((M, 0), np.int64)
            res.append(r)
        return res

    def stage_points(self, frames):
        """The points of a batch put where the library reads them, once, for several calls on the same frames (``staged=`` of
        run_batch, run_wide and inside_masks): what _stage_points returns.  Keep it until the last of those calls has returned."""
        return self._stage_points(frames)

    def run_batch(self, frames, want_uv=True, want_label=True, want_float=False, want_lists=True,
                  inst_cap=None, want_valid_uv=False, pinned=False, staged=None):
        """frames: list of f32[N_f,4] arrays, Scans of a ScanReader or float32 [N_f,4] GPU tensors (see _stage_points).  Returns one
        dict per frame with
        u, v (int32), label_bits, valid_idx, inst_lists, inst_count, count_mb, best_box, best_cnt,
        n_valid, n_labelled (+ depth, uf, vf with want_float; + u_valid, v_valid, label_valid with
        want_valid_uv: the values at the valid points only -- with want_uv/want_label off, a quarter of the read-back).
        pinned=True: the result arrays are views into page-locked buffers the context owns and reuses -- valid until the next
        run on this context (copy what must live longer); the frame loops use it.  staged: stage_points(frames), made by the caller."""
        off, pts_ptr, pts_dev, _keep = staged or self._stage_points(frames)      # (_keep: alive until the run returns)
        F, n = len(off) - 1, int(off[-1])
        M = self.M if self.F_masks else 0
        Btot = int(self.box_off[-1]) if self.box_off is not None else 0
        wants = dict(want_uv=want_uv, want_label=want_label, want_float=want_float, want_lists=want_lists, want_valid_uv=want_valid_uv)

        def launch(inst_cap):
            o = Outputs()
            finish = self._host_outputs(o, "", pinned, n, F, M, Btot, inst_cap, **wants)
            self._check(self._lib.lpf_run_batch(self._h, pts_ptr, off.ctypes.data, F, pts_dev, ctypes.byref(o)))
            return finish()

        out = self._until_lists_fit(launch, inst_cap, off)
        return self._frame_results(off, M, *out)

    _PER_POINT = {"uv": None, "label_bits": "label_bits", "label_words": "label_words", "depth": "depth", "u_f": "uf", "v_f": "vf"}
    _PER_VALID = ("valid_idx", "uv_valid", "label_valid", "label_valid_words")

    def _run_outputs(self, o, table, pinned, tag, inst_cap, null_if_empty):
        """Host result arrays of a run, wired into its outputs struct ``o`` (lpf_outputs or lpf_wide_outputs).  table: per field of
        ``o`` (field, shape, dtype, fill or None, wanted), in the order the result dicts list them.  pinned: the context's page-locked
        buffers (named tag + field), reused by the next run -- no allocation and no page faults per call, and the copies back are DMA
        transfers.  null_if_empty: an empty array is handed over as NULL (lpf_wide_outputs); lpf_outputs is given its address, as it
        always was -- the library reads NULL as "not wanted", so run_batch(inst_cap=0), which it refuses today ("inst_idx given with
        inst_cap=0"), would run without lists instead.  Returns finish(summary columns, last inst_off column, overflow flags) ->
        ((summary columns, per_point, per_valid, inst_idx, count_mb), 0 or the list capacity the run needed) for after the call."""
        a = {}
        for field, shape, dt, fill, wanted in table:
            if not wanted:
                arr = None
            elif pinned:
                arr = self._pinned(tag + field, shape, dt)
                if fill is not None:
                    arr[...] = fill
            else:
                arr = np.empty(shape, dt) if fill is None else np.full(shape, fill, dt)
            a[field] = arr
            setattr(o, field, arr.ctypes.data if (arr is not None and (arr.size or not null_if_empty)) else None)
        o.on_device, o.inst_cap = 0, inst_cap

        def finish(summ, last_off, overflow):
            per_point, per_valid = {}, {}
            for field, arr in a.items():
                if arr is None:
                    continue
                if field == "uv":
                    per_point.update(u=arr[:, 0], v=arr[:, 1])
                elif field == "uv_valid":
                    per_valid.update(uv_valid=arr, u_valid=arr[:, 0], v_valid=arr[:, 1])      # uv_valid: contiguous [n_valid, 2]
                elif field in self._PER_POINT:
                    per_point[self._PER_POINT[field]] = arr
                elif field in self._PER_VALID:
                    per_valid[field] = arr
            need = int(last_off.max()) if (a["inst_idx"] is not None and overflow.any()) else 0
            return (summ, per_point, per_valid, a["inst_idx"], a["count_mb"]), need
        return a, finish

    def _host_outputs(self, o, tag, pinned, n, F, M, Btot, inst_cap, want_uv, want_label, want_float, want_lists, want_valid_uv):
        """Host result arrays of a run (Ntot = n points, F frames, M masks, Btot boxes), wired into the lpf_outputs ``o``.  Returns
        finish() of _run_outputs, for after the call."""
        vu = want_valid_uv and want_lists                                     # only the first n_valid rows come back
        a, finish = self._run_outputs(o, (
            ("uv", (n, 2), np.int32, None, want_uv), ("label_bits", (n,), np.uint32, None, want_label),
            ("depth", (n,), np.float64, None, want_float), ("u_f", (n,), np.float64, None, want_float),
            ("v_f", (n,), np.float64, None, want_float), ("valid_idx", (n,), np.int64, None, want_lists),
            ("uv_valid", (n, 2), np.int32, None, vu), ("label_valid", (n,), np.uint32, None, vu),
            ("inst_idx", (F, inst_cap), np.int64, None, want_lists and M), ("count_mb", (max(M * Btot, 1),), np.int32, 0, True),
            ("summary", (F,), SUMMARY_DTYPE, 0, True)), pinned, tag, inst_cap, False)
        summ = a["summary"]
        return lambda: finish(summ, summ["inst_off"][:, 32], summ["inst_overflow"])

    def _cam_inputs(self, frames, cams, max_masks, who):
        """The lpf_cam_input array of a multi-camera pass over ``frames`` (run_cams' camera dicts), checked before anything reaches the
        GPU: (CamInput [C], masks per camera, box offsets per camera or None, what must stay alive until the run returns)."""
        C = len(cams)
        if not 1 <= C <= LPF_MAX_CAMS:
            raise ValueError("%s takes 1 to %d cameras, got %d" % (who, LPF_MAX_CAMS, C))
        F = len(frames)
        if F == 0:
            raise ValueError("no frames")
        cin = (CamInput * C)()
        keep, Ms, box_offs = [], [], []
        for k, cam in enumerate(cams):
            W, H = int(cam["width"]), int(cam["height"])
            T = np.ascontiguousarray(cam["T_velo_to_rect"], dtype=np.float64).reshape(-1)
            K = np.asarray(cam["K"], dtype=np.float64)
            if T.size != 16 or K.ndim != 2 or K.shape[0] < 3 or K.shape[1] < 3 or W <= 0 or H <= 0:
                raise ValueError("camera %d: T_velo_to_rect must be 4x4, K at least 3x3, width and height positive" % k)
            binarize = cam.get("binarize") or ("v3" if cam.get("v3_pipeline") else "astype")
            masks = cam.get("masks")
            if masks is None:
                masks = np.zeros((F, 0, H, W), np.uint8)
            erode = cam.get("erode_iters", 0)
            batch = compact_mask_batch(masks, F, H, W, cam.get("rects"), erode, binarize, max_masks, "%s: camera %d" % (who, k),
                                       forms=("rle",)) or \
                wide_mask_batch(masks, F, H, W, cam.get("rects"), erode, binarize, self.BINARIZE)
            M = batch.M
            if M > max_masks:
                raise ValueError("camera %d has %d masks per frame: a multi-camera pass takes at most %d per camera (run_wide takes more)"
                                 % (k, M, max_masks))
            ci = cin[k]
            ci.T_velo_to_rect[:] = T.tolist()
            ci.K[:] = np.ascontiguousarray(K[:3, :3]).reshape(9).tolist()
            ci.W, ci.H = W, H
            ci.depth_min_excl, ci.depth_max_excl = float(cam.get("depth_min", 0.0)), float(cam.get("depth_max", 50.0))
            self._wide_input(ci.masks, batch, binarize, erode)
            boxes, box_off = cam.get("boxes"), None
            if boxes is not None:
                if isinstance(boxes, np.ndarray) and F == 1:
                    boxes = [boxes]
                if len(boxes) != F:
                    raise ValueError("camera %d: boxes for %d frames, the batch has %d" % (k, len(boxes), F))
                arrs = [np.asarray(b, dtype=np.float64).reshape(-1, 8, 3) for b in boxes]
                box_off = np.zeros(F + 1, np.int32)
                box_off[1:] = np.cumsum([a.shape[0] for a in arrs])
                cat = np.ascontiguousarray(np.concatenate(arrs, axis=0))
                ci.corners_velo = cat.ctypes.data if cat.size else None
                ci.box_off = box_off.ctypes.data
                ci.boxes_on_device, ci.oriented = 0, int(bool(cam.get("oriented", True)))
                keep.append(cat)
            keep.append(batch)
            Ms.append(M)
            box_offs.append(box_off)
        return cin, Ms, box_offs, keep

    def run_cams(self, frames, cams, want_uv=True, want_label=True, want_float=False, want_lists=True, inst_cap=None,
                 want_valid_uv=False, pinned=False):
        """One batch of frames labelled in up to four cameras in ONE native pass (lpf_run_cams): the points are staged once (as
        run_batch's ``frames``: host arrays, Scans of a ScanReader, float32 [N,4] GPU tensors) and read once by the GPU.
        cams: one dict per camera --
          T_velo_to_rect  4x4, K  (3x3 or larger), width, height, depth_min (0.0), depth_max (50.0)  -- set_camera's arguments
          masks           [M,H,W] (one frame) or [F,M,H,W], uint8 / bool or float32, NumPy or a contiguous GPU tensor, M <= 32; or None;
                          or run-length: one rle.RleMasks, or a list with one per frame, at THIS camera's size (no rects, default
                          binarize; decoded on the GPU) -- cameras with dense masks and cameras with RleMasks may share a pass
          binarize        float masks: "astype" (default), "v3" or "gt0.5" (set_masks'); v3_pipeline=True means "v3"
          erode_iters     (0), rects: the optional [F,M,4] hint of set_mask_rects (where the masks are)
          boxes           one f64 [B_f,8,3] array of velodyne-frame corners per frame (set_boxes'), or None; oriented (True)
        Returns one list per camera of what run_batch returns for that camera after set_camera / set_mask_rects / set_masks /
        set_boxes with the same arguments -- equal, array for array.  The context's camera, masks and boxes are left as they were."""
        cin, Ms, box_offs, _keep_in = self._cam_inputs(frames, cams, LPF_MAX_MASKS, "run_cams")
        C, F = len(cams), len(frames)
        off, pts_ptr, pts_dev, _keep = self._stage_points(frames)      # (_keep: alive until the run returns)
        n = int(off[-1])
        wants = dict(want_uv=want_uv, want_label=want_label, want_float=want_float, want_lists=want_lists, want_valid_uv=want_valid_uv)

        def launch(inst_cap):
            outs = (Outputs * C)()
            fins = [self._host_outputs(outs[k], "cam%d_" % k, pinned, n, F, Ms[k], int(box_offs[k][-1]) if box_offs[k] is not None else 0,
                                       inst_cap, **wants) for k in range(C)]
            self._check(self._lib.lpf_run_cams(self._h, pts_ptr, off.ctypes.data, F, pts_dev, cin, C, outs))
            res = [fin() for fin in fins]
            return [r for r, _ in res], max(need for _, need in res)

        outs = self._until_lists_fit(launch, inst_cap, off)
        return [self._frame_results(off, Ms[k], *outs[k], box_off=box_offs[k]) for k in range(C)]

    def _wide_host_outputs(self, o, n, F, M, Btot, inst_cap, want_uv, want_float, want_lists, want_valid_uv, want_label=True, pinned=False,
                           tag=""):
        """Host result arrays of a wide run (Ntot = n points, F frames, M masks, Btot boxes), wired into the lpf_wide_outputs ``o``.
        Returns finish() of _run_outputs, for after the call.  want_label=False: no dense label_words."""
        LW = (M + 31) // 32
        vu = want_valid_uv and want_lists
        a, finish = self._run_outputs(o, (
            ("label_words", (n, LW), np.uint32, None, want_label), ("uv", (n, 2), np.int32, None, want_uv),
            ("depth", (n,), np.float64, None, want_float), ("u_f", (n,), np.float64, None, want_float),
            ("v_f", (n,), np.float64, None, want_float), ("valid_idx", (n,), np.int64, None, want_lists),
            ("uv_valid", (n, 2), np.int32, None, vu), ("label_valid_words", (n, LW), np.uint32, None, vu),
            ("inst_idx", (F, inst_cap), np.int64, None, want_lists and M), ("count_mb", (max(M * Btot, 1),), np.int32, 0, True),
            ("n_valid", (F,), np.int64, 0, True), ("n_labelled", (F,), np.int64, 0, True), ("inst_count", (F, M), np.int64, 0, True),
            ("inst_off", (F, M + 1), np.int64, 0, True), ("best_cnt", (F, M), np.int64, 0, True), ("best_box", (F, M), np.int32, -1, True),
            ("inst_overflow", (F,), np.int32, 0, True)), pinned, tag + "w_", inst_cap, True)
        summ = {k: a[k] for k in ("n_valid", "n_labelled", "inst_count", "inst_off", "best_box", "best_cnt")}
        return lambda: finish(summ, a["inst_off"][:, M], a["inst_overflow"])

    def _wait_for_masks(self, batch):
        """Masks and maps on the GPU were produced on torch's stream: the call that reads them is ordered after it"""
        if batch.gpu is not None:
            import torch
            self.wait_for_stream(torch.cuda.current_stream(batch.gpu.device).cuda_stream)

    def _wide_input(self, inp, batch, binarize, erode_iters):
        """Fills the lpf_wide_input ``inp`` from a MaskBatch (which must stay alive until the call has returned) and orders the call
        after the stream that made GPU masks: dense masks, or the run-length form, which rides in this struct as LPF_MASKS_RLE -- its
        ``masks`` is the lpf_rle_masks itself, in host memory (no M = 0 shortcut: the struct says so itself)."""
        self._wait_for_masks(batch)
        M = batch.M
        if batch.form == "rle":
            inp.masks, inp.f32, inp.binarize = ctypes.addressof(batch.struct), LPF_MASKS_RLE, 0
        else:
            inp.masks, inp.f32, inp.binarize = _ptr(batch.masks) if M else None, int(batch.is_float), self.BINARIZE[binarize]
        inp.rects = _ptr(batch.rects) if M else None
        inp.M, inp.erode_iters, inp.on_device = M, int(erode_iters), 1 if batch.on_device else 0

    def _masks_call(self, batch, binarize, erode_iters, natives):
        """The native call a pass makes for its masks.  natives: the functions the entry point has, by form -- "dense" takes a
        lpf_wide_input, and a compact form without a function of its own rides in that struct; a compact form with one takes the struct
        compact_mask_batch made.  Returns ``(function, input struct, what must stay alive until the call has returned)``, with the
        wait for the stream that made GPU masks or maps done."""
        if batch.form != "dense" and batch.form in natives:
            self._wait_for_masks(batch)
            return natives[batch.form], batch.struct, batch
        inp = WideInput()
        self._wide_input(inp, batch, binarize, erode_iters)
        return natives["dense"], inp, batch

    def run_wide(self, frames, masks, erode_iters=0, binarize="astype", rects=None, v3_pipeline=False, want_uv=True, want_float=False,
                 want_lists=True, want_valid_uv=False, inst_cap=None, staged=None):
        """Frames with up to 256 masks each in ONE native pass (lpf_run_wide): every point is projected and read once.
        frames: as run_batch's -- f32[N_f,4] host arrays, Scans of a ScanReader (read in HBM where they are), float32 [N,4] GPU
        tensors.  masks: [M,H,W] or [F,M,H,W] (uint8 / bool, or
        float32 under ``binarize`` as set_masks), host or GPU (lent until the call returns: it waits for its results); or in run-length
        form -- one rle.RleMasks, or a list with one per frame (ragged M is padded with empty masks), at the camera's size, without
        ``rects`` and under the default ``binarize``: the runs are decoded into the label planes on the GPU, nothing dense crosses to the
        device, and every result equals the one ``.to_dense()`` masks give; or as instance-ID maps -- one idmap.IdMasks, or a list with
        one per frame (ragged M is padded with LPF_ID_NONE), under set_masks_ids' rules: lpf_run_wide_ids builds the label planes from
        the map on the GPU, with the same results as ``.to_dense()`` masks.  rects: the
        optional [F,M,4] hint of set_mask_rects.  Boxes and camera are the ones in force; the masks, boxes and rectangles of the
        narrow calls are left as they are.  Returns one dict per frame with what run_batch returns -- inst_count, best_box,
        best_cnt of length M, count_mb [M, B_f] -- plus label_words [N_f, LW] (bit b of word w = mask 32 w + b; LW = ceil(M / 32)),
        and with want_valid_uv label_valid_words [n_valid, LW].  staged: stage_points(frames), made by the caller."""
        if v3_pipeline:
            binarize = "v3"
        F = len(frames)
        if F == 0:
            raise ValueError("no frames")
        batch = compact_mask_batch(masks, F, self.H, self.W, rects, erode_iters, binarize, forms=("ids", "rle")) or \
            wide_mask_batch(masks, F, self.H, self.W, rects, erode_iters, binarize, self.BINARIZE)
        M = batch.M
        off, pts_ptr, pts_dev, _keep = staged or self._stage_points(frames)      # (_keep: alive until the run returns)
        n = int(off[-1])
        native, inp, _keep_masks = self._masks_call(batch, binarize, erode_iters,
                                                    {"dense": self._lib.lpf_run_wide, "ids": self._lib.lpf_run_wide_ids})
        Btot = int(self.box_off[-1]) if self.box_off is not None else 0
        wants = dict(want_uv=want_uv, want_float=want_float, want_lists=want_lists, want_valid_uv=want_valid_uv)

        def launch(inst_cap):
            o = WideOutputs()
            finish = self._wide_host_outputs(o, n, F, M, Btot, inst_cap, **wants)
            self._check(native(self._h, pts_ptr, off.ctypes.data, F, pts_dev, ctypes.byref(inp), ctypes.byref(o)))
            return finish()

        out = self._until_lists_fit(launch, inst_cap, off)
        return self._frame_results(off, M, *out)

    _DEPTH_MAPS_OUT = {"pix": "int64", "depth": "float64", "point_idx": "int64", "car_off": "int64", "need": "int64", "overflow": "int32"}

    def depth_maps(self, frames, masks, binarize="gt0.5", rects=None, erode_iters=0, cap=None, want_point_idx=True, out=None):
        """seg_with_pointcloud's per-car depth maps of a batch of frames in ONE native call (lpf_depth_maps) and one host wait.
        frames: as run_wide's -- f32[N_f,4] host arrays, Scans of a ScanReader, float32 [N,4] GPU tensors.  masks: [M,H,W] or
        [F,M,H,W] at the camera's size (uint8 / bool: nonzero, or float32 under ``binarize``; "gt0.5" is the script's mask > 0.5),
        host or GPU; or in run-length form -- one rle.RleMasks, or a list with one per frame (ragged M is padded with empty masks), at
        the camera's size, without ``rects`` and under the default ``binarize`` (lpf_depth_maps_rle: the runs are decoded into label
        planes on the GPU, nothing dense crosses to the device, every result equals the one ``.to_dense()`` masks give);
        rects: the optional [F,M,4] hint of set_mask_rects; erode_iters: cv2.erode iterations.  The camera, transform
        and depth window are set_camera's.  Returns, per frame, M tuples (pix int64, depth float64, point_idx int64 or None): car m
        = np.flatnonzero(np.where(member_m, D, 0)) with D the frame's depth_image, its depths and the winning points.  cap: list
        entries per frame of the first attempt (default from the point counts); a frame that needs more runs the call once more
        with the exact capacity.
        out: the caller's own GPU tensors for lpf_depth_maps_outputs -- "pix", "depth", "point_idx" [at least F, cap] (depth and point_idx
        may be left out), "car_off" int64 [F, M + 1], "need" int64 [F], "overflow" int32 [F] (may be left out) -- with ``cap`` given:
        ONE call in torch's stream order, no second attempt, nothing read back; entries at or beyond cap and beyond a frame's need are
        not written (include/lpf.h).  Returns ``out``."""
        F = len(frames)
        if F == 0:
            raise ValueError("no frames")
        if cap is not None and (isinstance(cap, bool) or int(cap) != cap or cap < 0):
            raise ValueError("cap must be a non-negative integer, got %r" % (cap,))
        batch = compact_mask_batch(masks, F, self.H, self.W, rects, erode_iters, binarize, who="depth_maps", default_binarize="gt0.5",
                                   forms=("rle",)) or \
            wide_mask_batch(masks, F, self.H, self.W, rects, erode_iters, binarize, self.BINARIZE)
        M = batch.M
        off, pts_ptr, pts_dev, _keep = self._stage_points(frames)      # (_keep: alive until the call returns)
        native, inp, _keep_masks = self._masks_call(batch, binarize, erode_iters,
                                                    {"dense": self._lib.lpf_depth_maps, "rle": self._lib.lpf_depth_maps_rle})
        if out is not None:
            if cap is None or int(cap) < 1:
                raise ValueError("depth_maps: out= needs a capacity of at least one entry")
            unknown = set(out) - set(self._DEPTH_MAPS_OUT)
            if unknown or "pix" not in out or "car_off" not in out or "need" not in out:
                raise ValueError("depth_maps: out= holds pix, car_off, need and optionally depth, point_idx, overflow; got %s" % sorted(out))
            for k, t in out.items():
                rows = k in ("pix", "depth", "point_idx")
                want = (F, int(cap)) if rows else (F, M + 1) if k == "car_off" else (F,)
                shape = tuple(t.shape)
                if not (_is_torch(t) and t.is_cuda and t.is_contiguous()) or len(shape) != len(want) or shape[1:] != want[1:] or \
                        (shape[0] < F if rows else shape[0] != F):
                    raise ValueError("depth_maps: out[%r] must be a contiguous GPU tensor %s, got %s" % (k, want, shape))
            o = DepthMapsOutputs()
            for k, dt in self._DEPTH_MAPS_OUT.items():
                setattr(o, k, _dev_ptr(out.get(k), dt))
            o.cap, o.on_device = int(cap), 1
            self._call_in_order(out["pix"].device, native, pts_ptr, off.ctypes.data, F, pts_dev, ctypes.byref(inp), ctypes.byref(o))
            self._lent.append((_keep, _keep_masks))     # (staged points and masks: alive until the work has run)
            return out
        if cap is None:                     # a quarter of the largest frame's points: frame 100's five cars are 8 k of its 109 k
            cap = 0 if M == 0 else max(1024, min(int(np.diff(off).max()) // 4, self.W * self.H))

        def launch(cap):
            o = DepthMapsOutputs()
            pix = self._pinned("dm_pix", (F, cap), np.int64)
            dep = self._pinned("dm_dep", (F, cap), np.float64)
            pid = self._pinned("dm_pid", (F, cap), np.int64) if want_point_idx else None
            car_off, need, ovf = np.zeros((F, M + 1), np.int64), np.zeros(F, np.int64), np.zeros(F, np.int32)
            o.pix, o.depth = (pix.ctypes.data, dep.ctypes.data) if cap else (None, None)
            o.point_idx = pid.ctypes.data if (pid is not None and cap) else None
            o.cap, o.car_off, o.need, o.overflow, o.on_device = cap, car_off.ctypes.data, need.ctypes.data, ovf.ctypes.data, 0
            self._check(native(self._h, pts_ptr, off.ctypes.data, F, pts_dev, ctypes.byref(inp), ctypes.byref(o)))
            return pix, dep, pid, car_off, need, ovf

        pix, dep, pid, car_off, need, ovf = launch(int(cap))
        if ovf.any():                       # once, with the exact capacity
            pix, dep, pid, car_off, need, ovf = launch(int(need.max()))
        out = []
        for f in range(F):
            o = car_off[f]
            out.append([(pix[f, o[m]:o[m + 1]].copy(), dep[f, o[m]:o[m + 1]].copy(),
                         pid[f, o[m]:o[m + 1]].copy() if pid is not None else None) for m in range(M)])
        return out

    @staticmethod
    def overlay_rows(maps, hw):
        """depth_maps()' per-frame car lists -> the rows of lpf_depth_overlay_input: pix int64 [F,cap], depth float64 [F,cap], car_off
        int64 [F,M+1] and M.  Every car must be a strictly ascending pixel list inside the image with finite depths > 0 (ValueError)."""
        F = len(maps)
        Ms = {len(cars) for cars in maps}
        if len(Ms) > 1:
            raise ValueError("every frame of depth maps must have the same number of cars, got %s" % sorted(Ms))
        M = Ms.pop() if Ms else 0
        if M > LPF_MAX_MASKS_WIDE:
            raise ValueError("M=%d cars per frame, depth_overlays takes at most %d" % (M, LPF_MAX_MASKS_WIDE))
        car_off = np.zeros((F, M + 1), np.int64)
        cars = []
        for f, fr in enumerate(maps):
            for m, car in enumerate(fr):
                pix, dep = np.asarray(car[0]), np.asarray(car[1])
                if pix.ndim != 1 or dep.shape != pix.shape or pix.dtype.kind not in "iu" or dep.dtype.kind != "f":
                    raise ValueError("frame %d car %d: pixels must be an integer list and depths a float list of the same length" % (f, m))
                if len(pix) and (pix[0] < 0 or pix[-1] >= hw or (len(pix) > 1 and not (np.diff(pix) > 0).all())):
                    raise ValueError("frame %d car %d: pixels must be strictly ascending inside the image [0, %d)" % (f, m, hw))
                if len(dep) and not (np.isfinite(dep).all() and (dep > 0).all()):
                    raise ValueError("frame %d car %d: depths must be finite and > 0" % (f, m))
                car_off[f, m + 1] = car_off[f, m] + len(pix)
                cars.append((f, m, pix, dep))
        cap = int(car_off[:, -1].max()) if F else 0
        pix_rows, dep_rows = np.zeros((F, cap), np.int64), np.zeros((F, cap), np.float64)
        for f, m, pix, dep in cars:
            pix_rows[f, car_off[f, m]:car_off[f, m + 1]] = pix
            dep_rows[f, car_off[f, m]:car_off[f, m + 1]] = dep
        return pix_rows, dep_rows, car_off, M

    @staticmethod
    def _want(who, want, known):
        """the selection ``want`` of an analysis call's outputs ``known``, as a tuple"""
        want = tuple(want)
        if not want or any(w not in known for w in want):
            raise ValueError("%s: want is a selection of %s, got %r" % (who, known, want))
        return want

    @staticmethod
    def _on_gpu(who, arrays, noun):
        """True when every one of an analysis call's ``arrays`` is a GPU tensor, False when none is"""
        n_dev = sum(1 for a in arrays if _is_torch(a) and a.is_cuda)
        if n_dev not in (0, len(arrays)):
            raise ValueError("%s: host arrays and GPU tensors are mixed (%d of %d %s are on the GPU)" % (who, n_dev, len(arrays), noun))
        return n_dev > 0

    @staticmethod
    def _outputs(who, o, names, table, dims, device, out=None, fields=None):
        """The outputs ``names`` of an analysis call, wired into its outputs struct ``o`` (field fields[name], or name): GPU tensors on
        ``device``, NumPy arrays for device None.  table: name -> (dtype, shape with the sizes of ``dims`` by name, fill; None: left
        as allocated).  out: the caller's own arrays under the same names, taken as they are when they fit the table."""
        dev = device is not None
        if dev:
            import torch
        mod = torch if dev else np
        res = {}
        for w in names:
            dt, shape, fill = table[w]
            shape = tuple(map(dims.get, shape, shape))          # (a size by its name, a number as it is)
            a = out.get(w) if out else None
            if a is None:                                   # (fresh and contiguous: nothing to check)
                make = mod.empty if fill is None else mod.zeros if fill == 0 else mod.full
                args = (shape,) if fill is None or fill == 0 else (shape, fill)
                a = make(*args, dtype=getattr(torch, dt), device=device) if dev else make(*args, dt)
            elif dev:
                if tuple(a.shape) != shape:
                    raise ValueError("%s: out[%r] must be %s, got %s" % (who, w, shape, tuple(a.shape)))
                _dev_ptr(a, dt)
            elif a.shape != shape or a.dtype != np.dtype(dt) or not a.flags.c_contiguous:
                raise ValueError("%s: out[%r] must be a contiguous %s array %s" % (who, w, dt, shape))
            res[w] = a
            setattr(o, fields.get(w, w) if fields else w, _ptr(a))
        o.on_device = int(dev)
        return res

    _OVERLAY_OUT = {"images": ("uint8", ("F", "M", "H", "W", 3), None), "max_depth": ("float64", ("F", "M"), 0)}

    def depth_overlays(self, maps, seg_images):
        """seg_with_pointcloud.py:174-180's per-car overlay images in ONE native call (lpf_depth_overlays): ``maps`` is what
        depth_maps() returns (per frame, M tuples (pix, depth, ...)), ``seg_images`` the segmented images uint8 [F,H,W,3] at the
        camera's size (set_camera), a NumPy array or a GPU tensor.  Returns (images uint8 [F,M,H,W,3], max_depth float64 [F,M]):
        image (f, m) is the script's cvtColor(np.uint8(image_withseg * 255), COLOR_RGB2BGR) byte for byte, max_depth its
        np.max(depthMap) (0 for an empty car, whose image is only the reversed segmented image: the script skips that car).  Host
        images give NumPy outputs after one host wait; a GPU tensor gives torch tensors on its device, in torch's stream order
        (the call only enqueues work)."""
        dev = _is_torch(seg_images)
        F = len(maps)
        shape = (F, self.H, self.W, 3)
        if tuple(seg_images.shape) != shape:
            raise ValueError("segmented images must be uint8 [F,H,W,3] = %s at the camera's size, got %s" % (shape, tuple(seg_images.shape)))
        if str(seg_images.dtype) not in ("torch.uint8", "uint8"):
            raise ValueError("segmented images must be uint8, got %s" % (seg_images.dtype,))
        lists = self.overlay_rows(maps, self.W * self.H)
        M = lists[3]
        if dev:
            import torch
            device = seg_images.device
            seg = seg_images.contiguous()
            pix, dep, car_off = (torch.from_numpy(a).to(device) for a in lists[:3])
        else:
            device = None
            seg = np.ascontiguousarray(seg_images)
            pix, dep, car_off = lists[:3]
        inp, o = DepthOverlayInput(), DepthOverlayOutputs()
        res = self._outputs("depth_overlays", o, ("images", "max_depth"), self._OVERLAY_OUT, dict(F=F, M=M, H=self.H, W=self.W), device)
        if F and M:
            inp.cap, inp.M = pix.shape[1], M
            inp.pix, inp.depth, inp.car_off, inp.seg = _ptr(pix), _ptr(dep), _ptr(car_off), _ptr(seg)
            inp.lists_on_device = inp.seg_on_device = o.on_device
            self._call_in_order(device, self._lib.lpf_depth_overlays, F, ctypes.byref(inp), ctypes.byref(o))
        return res["images"], res["max_depth"]

    MATCH2D_WANT = ("best", "iou", "center", "size", "total", "cost")
    _MATCH2D_FIELD = {"center": "center_score", "size": "size_score", "total": "total_score"}
    _MATCH2D_OUT = {"best_box": ("int32", ("D",), -1), "best_iou": ("float64", ("D",), 0), "iou": ("float64", ("P",), None),
                    "center": ("float64", ("P",), None), "size": ("float64", ("P",), None), "total": ("float64", ("P",), None),
                    "cost": ("float64", ("P",), None)}

    @staticmethod
    def _pair_offsets(who, rows, cols, nouns):
        """The int32 [F+1] offsets (det_off, box_off) of a batch from its per-frame row and column counts; ValueError where either sum
        does not fit (nouns: what ``who`` calls rows and columns)."""
        det_off, box_off = (np.concatenate([[0], np.cumsum(n, dtype=np.int64)]) for n in (rows, cols))
        if det_off[-1] > 0x7fffffff or box_off[-1] > 0x7fffffff:
            raise ValueError("%s: %d %s and %d %s, a call takes fewer than 2^31 of each" % (who, det_off[-1], nouns[0], box_off[-1], nouns[1]))
        return det_off.astype(np.int32), box_off.astype(np.int32)

    @staticmethod
    def match2d_batch(dets, bbox2d, front):
        """The per-frame lists of match_2d checked and described: (on_device, dets dtype name, det_off int32 [F+1], box_off int32
        [F+1]).  ValueError for frame counts that differ, detections that are not float32 / float64 [D,4] of one dtype, rectangles that
        are not [B,4], front counts that are not [B], and host arrays mixed with GPU tensors."""
        dets, bbox2d, front = list(dets), list(bbox2d), list(front)
        if not (len(dets) == len(bbox2d) == len(front)):
            raise ValueError("match_2d: one entry per frame in each list, got %d detections, %d bbox2d, %d front" % (len(dets), len(bbox2d), len(front)))
        dev = LpfContext._on_gpu("match_2d", dets + bbox2d + front, "inputs")
        name = lambda a: str(a.dtype).replace("torch.", "")
        dtypes, D, B = set(), [], []
        for f, (d, b, fr) in enumerate(zip(dets, bbox2d, front)):
            if not dev:
                d, b, fr = np.asarray(d), np.asarray(b), np.asarray(fr)
            if len(d.shape) != 2 or d.shape[1] != 4:
                raise ValueError("match_2d: frame %d: detections must be [D,4] (x1, y1, x2, y2), got %s" % (f, tuple(d.shape)))
            if name(d) not in ("float32", "float64"):
                raise ValueError("match_2d: frame %d: detections must be float32 or float64, got %s" % (f, name(d)))
            dtypes.add(name(d))
            if len(b.shape) != 2 or b.shape[1] != 4:
                raise ValueError("match_2d: frame %d: bbox2d must be [B,4] (min u, min v, max u, max v), got %s" % (f, tuple(b.shape)))
            if tuple(fr.shape) != (b.shape[0],):
                raise ValueError("match_2d: frame %d: front must be [B] = [%d], got %s" % (f, b.shape[0], tuple(fr.shape)))
            if dev and (name(b) != "float64" or name(fr) != "int32"):
                raise ValueError("match_2d: frame %d: GPU bbox2d must be float64 and front int32, got %s and %s" % (f, name(b), name(fr)))
            if not dev and (np.asarray(b).dtype.kind not in "fiu" or np.asarray(fr).dtype.kind not in "iub"):
                raise ValueError("match_2d: frame %d: bbox2d must be numbers and front integers, got %s and %s" % (f, name(b), name(fr)))
            D.append(d.shape[0])
            B.append(b.shape[0])
        if len(dtypes) > 1:
            raise ValueError("match_2d: the detections of a call share one dtype, got %s" % sorted(dtypes))
        return (dev, dtypes.pop() if dtypes else "float32", *LpfContext._pair_offsets("match_2d", D, B, ("detections", "boxes")))

    def _match2d_input(self, dets, bbox2d, front, min_iou, weights):
        """What match_2d and assign_2d hand to the library for their per-frame lists: (the filled Match2dInput, the torch device or None
        for host arrays, det_off, box_off, the concatenated arrays behind the struct's pointers -- the caller holds them across the
        call)."""
        dets, bbox2d, front = list(dets), list(bbox2d), list(front)
        dev, dt, det_off, box_off = self.match2d_batch(dets, bbox2d, front)
        Dtot, Btot = int(det_off[-1]), int(box_off[-1])
        device = dd = bb = ff = None
        if dev:
            import torch
            device = dets[0].device
            if Dtot:
                dd = torch.cat([x.reshape(-1, 4) for x in dets]).contiguous()
            if Btot:
                bb, ff = torch.cat([x.reshape(-1, 4) for x in bbox2d]).contiguous(), torch.cat(front).contiguous()
        else:
            if Dtot:
                dd = np.ascontiguousarray(np.concatenate([np.asarray(x).reshape(-1, 4) for x in dets]), dtype=dt)
            if Btot:
                bb = np.ascontiguousarray(np.concatenate([np.asarray(x).reshape(-1, 4) for x in bbox2d]), dtype=np.float64)
                ff = np.ascontiguousarray(np.concatenate([np.asarray(x) for x in front]), dtype=np.int32)
        inp = Match2dInput()
        inp.dets, inp.bbox2d, inp.front, inp.det_off, inp.box_off = _ptr(dd), _ptr(bb), _ptr(ff), det_off.ctypes.data, box_off.ctypes.data
        inp.dets_f64, inp.on_device = int(dt == "float64"), int(dev)
        inp.min_iou, (inp.w_iou, inp.w_center, inp.w_size) = float(min_iou), weights
        return inp, device, det_off, box_off, (dd, bb, ff)

    def match_2d(self, dets, bbox2d, front, min_iou=0.25, weights=(0.5, 0.3, 0.2), want=("best",)):
        """V4's and V5's detection-to-box scoring for a batch of frames in ONE native call (lpf_match_2d).  Per frame: ``dets`` [D,4]
        float32 (the detector's boxes.xyxy) or float64, ``bbox2d`` float64 [B,4] and ``front`` int32 [B] as prepare_boxes returns them;
        all host arrays or all GPU tensors.  ``want`` picks the outputs: "best" (V4: best_box int32 [D], the first strict maximum of the
        IoU above min_iou into the frame's boxes or -1, and best_iou float64 [D]) and the [D,B] float64 matrices "iou", "center",
        "size", "total", "cost" of V5 (cost = 1 - total: what V5 hands to linear_sum_assignment; a column of a box with front == 0 is
        iou 0, scores 0, cost 1).  Returns a dict of per-frame lists, keys "best_box", "best_iou" and the matrices' names.  The
        arithmetic is the reference's, type for type (include/lpf.h).  Host arrays: NumPy results after one host wait; GPU tensors:
        torch tensors on their device in torch's stream order (the call only enqueues work)."""
        want = self._want("match_2d", want, self.MATCH2D_WANT)
        weights = tuple(float(w) for w in weights)
        if len(weights) != 3 or not all(np.isfinite(weights)) or not np.isfinite(float(min_iou)):
            raise ValueError("match_2d: min_iou and the three weights (iou, center, size) must be finite numbers")
        inp, device, det_off, box_off, held = self._match2d_input(dets, bbox2d, front, min_iou, weights)
        F, Dtot = len(det_off) - 1, int(det_off[-1])
        D, B = np.diff(det_off).astype(np.int64), np.diff(box_off).astype(np.int64)
        pair_off = np.concatenate([[0], np.cumsum(D * B)]).astype(np.int64)
        mats = [w for w in want if w != "best"]
        o = Match2dOutputs()
        flat = self._outputs("match_2d", o, (["best_box", "best_iou"] if "best" in want else []) + mats, self._MATCH2D_OUT,
                             dict(D=Dtot, P=int(pair_off[-1])), device, fields=self._MATCH2D_FIELD)
        if F and Dtot:
            self._call_in_order(device, self._lib.lpf_match_2d, F, ctypes.byref(inp), ctypes.byref(o))
        res = {k: [flat[k][det_off[f]:det_off[f + 1]] for f in range(F)] for k in ("best_box", "best_iou") if k in flat}
        for w in mats:
            res[w] = [flat[w][pair_off[f]:pair_off[f + 1]].reshape(int(D[f]), int(B[f])) for f in range(F)]
        return res

    ASSIGN_MESSAGES = {1: "matrix contains invalid numeric entries", 2: "cost matrix is infeasible"}     # SciPy's two
    _ASSIGN_OUT = {"col_of_row": ("int32", ("D",), -1), "status": ("int32", ("F",), 0)}

    def assign_costs(self, costs, front=None, raw=False):
        """scipy.optimize.linear_sum_assignment for a batch of cost matrices in ONE native call (lpf_assign_costs): ``costs`` is a
        list of per-frame [D,B] float64 arrays, or of GPU tensors; ``front`` None or a list of per-frame [B] integers -- a column
        with front <= 0 is dropped before the assignment (V5:337-341), the returned columns stay in original numbering.  Returns per
        frame ``(rows, cols)`` as int64 NumPy arrays, exactly linear_sum_assignment's return (SciPy's tie-breaking, not merely an
        optimal assignment).  ValueError with SciPy's message and the frame for a frame whose live entries hold a NaN or -inf
        ("matrix contains invalid numeric entries") or that has no complete assignment ("cost matrix is infeasible"); LpfError
        (LPF_ERR_ARG, naming the frame) for a frame beyond LPF_ASSIGN_MAX rows or live columns.  raw=True: the dict {"col_of_row": int32 [Dtot], "status": int32 [F]} as the
        call wrote it -- with GPU tensors the call only enqueues work, in torch's stream order, and nothing is waited for."""
        costs = list(costs)
        F = len(costs)
        fronts = None if front is None else list(front)
        if fronts is not None and len(fronts) != F:
            raise ValueError("assign_costs: one entry per frame in each list, got %d costs and %d front" % (F, len(fronts)))
        dev = self._on_gpu("assign_costs", costs + (fronts or []), "inputs")
        name = lambda a: str(a.dtype).replace("torch.", "")
        if not dev:
            costs = [np.asarray(m) for m in costs]
            fronts = None if fronts is None else [np.asarray(a) for a in fronts]
        for f, m in enumerate(costs):
            if len(m.shape) != 2:
                raise ValueError("assign_costs: frame %d: a cost matrix is [D,B], got %s" % (f, tuple(m.shape)))
            if dev and name(m) != "float64":
                raise ValueError("assign_costs: frame %d: GPU costs must be float64, got %s" % (f, name(m)))
            if not dev and m.dtype.kind not in "fiub":
                raise ValueError("assign_costs: frame %d: costs must be numbers, got %s" % (f, m.dtype))
            if fronts is not None:
                fr = fronts[f]
                if tuple(fr.shape) != (m.shape[1],):
                    raise ValueError("assign_costs: frame %d: front must be [B] = [%d], got %s" % (f, m.shape[1], tuple(fr.shape)))
                if (dev and name(fr) != "int32") or (not dev and fr.dtype.kind not in "iub"):
                    raise ValueError("assign_costs: frame %d: front must be integers (int32 on the GPU), got %s" % (f, name(fr)))
        det_off, box_off = self._pair_offsets("assign_costs", [m.shape[0] for m in costs], [m.shape[1] for m in costs], ("rows", "columns"))
        Dtot, Btot = int(det_off[-1]), int(box_off[-1])
        device = cc = ff = None
        if dev:
            import torch
            device = costs[0].device
            cc = torch.cat([m.reshape(-1) for m in costs]).contiguous()
            if fronts is not None and Btot:
                ff = torch.cat(fronts).contiguous()
        else:
            if F:
                cc = np.ascontiguousarray(np.concatenate([m.reshape(-1) for m in costs]), dtype=np.float64)
            if fronts is not None and Btot:
                ff = np.ascontiguousarray(np.concatenate(fronts), dtype=np.int32)
        inp, o = AssignInput(), AssignOutputs()
        res = self._outputs("assign_costs", o, ("col_of_row", "status"), self._ASSIGN_OUT, dict(D=Dtot, F=F), device)
        inp.cost, inp.front, inp.det_off, inp.box_off, inp.on_device = _ptr(cc), _ptr(ff), det_off.ctypes.data, box_off.ctypes.data, o.on_device
        if F:
            self._call_in_order(device, self._lib.lpf_assign_costs, F, ctypes.byref(inp), ctypes.byref(o))
        if raw:
            return res
        col, status = (a.cpu().numpy() if dev else a for a in (res["col_of_row"], res["status"]))
        out = []
        for f in range(F):
            if status[f]:
                raise ValueError("assign_costs: frame %d: %s" % (f, self.ASSIGN_MESSAGES.get(int(status[f]), "status %d" % status[f])))
            c = col[det_off[f]:det_off[f + 1]]
            rows = np.flatnonzero(c >= 0)
            out.append((rows.astype(np.int64), c[rows].astype(np.int64)))
        return out

    ASSIGN2D_WANT = ("box_of_det", "iou", "center", "size", "total", "accepted", "status")
    _ASSIGN2D_OUT = {"box_of_det": ("int32", ("D",), -1), "iou": ("float64", ("D",), 0), "center": ("float64", ("D",), 0),
                     "size": ("float64", ("D",), 0), "total": ("float64", ("D",), 0), "accepted": ("int32", ("D",), 0),
                     "status": ("int32", ("F",), 0)}

    def assign_2d(self, dets, bbox2d, front, weights=(0.5, 0.3, 0.2), min_score_threshold=0.3, min_iou_threshold=0.15, want=ASSIGN2D_WANT):
        """V5's matcher from detections and rectangles to accepted pairs for a batch of frames in ONE native call (lpf_assign_2d):
        the pair scores of match_2d, SciPy's linear_sum_assignment on the cost matrix of the boxes with front > 0 and the thresholds,
        all on the GPU -- no [D,B] matrix leaves it.  The inputs are match_2d's.  ``want`` picks the outputs (ASSIGN2D_WANT): per
        detection "box_of_det" int32 (an index into the frame's boxes, -1: none), the scores "iou", "center", "size", "total" float64
        of the assigned pair (match_2d's matrix entries bit for bit, 0 where none) and "accepted" int32 (total >=
        min_score_threshold and iou >= min_iou_threshold, V5:368); per frame "status" int32 (0 solved, 1 invalid entries, 2
        infeasible: nothing assigned).  Returns a dict: per-frame lists, and "status" as one [F] array.  Host arrays: NumPy results
        after one host wait; GPU tensors: torch tensors on their device in torch's stream order (the call only enqueues work).
        LpfError (LPF_ERR_ARG, naming the frame) for a frame beyond LPF_ASSIGN_MAX detections or boxes (live boxes, for host
        arrays)."""
        want = self._want("assign_2d", want, self.ASSIGN2D_WANT)
        weights = tuple(float(w) for w in weights)
        thr = (float(min_score_threshold), float(min_iou_threshold))
        if len(weights) != 3 or not all(np.isfinite(weights)) or any(np.isnan(thr)):
            raise ValueError("assign_2d: the three weights (iou, center, size) must be finite and the two thresholds numbers")
        inp, device, det_off, box_off, held = self._match2d_input(dets, bbox2d, front, 0.0, weights)
        F = len(det_off) - 1
        prm, o = Assign2dParams(*thr), Assign2dOutputs()
        flat = self._outputs("assign_2d", o, want, self._ASSIGN2D_OUT, dict(D=int(det_off[-1]), F=F), device, fields=self._MATCH2D_FIELD)
        if F:
            self._call_in_order(device, self._lib.lpf_assign_2d, F, ctypes.byref(inp), ctypes.byref(prm), ctypes.byref(o))
        res = {k: [flat[k][det_off[f]:det_off[f + 1]] for f in range(F)] for k in want if k != "status"}
        if "status" in want:
            res["status"] = flat["status"]
        return res

    INSIDE_WANT = ("inside", "part_idx", "part_xyz", "n_inside", "matched")
    _INSIDE_OUT = {"inside": ("uint8", ("F", "cap"), 0), "part_idx": ("int64", ("F", "cap"), 0), "part_xyz": ("float32", ("F", "cap", 3), 0),
                   "n_inside": ("int64", ("F", "M"), 0), "matched": ("int32", ("F", "M"), 0)}

    @staticmethod
    def inside_batch(inst_idx, inst_off, best_box, best_cnt):
        """The four list arrays of inside_masks checked and described: (on_device, F, M, inst_cap).  ValueError for host arrays mixed
        with GPU tensors, GPU tensors of another dtype than int64 / int64 / int32 / int64, and shapes that are not [F, inst_cap],
        [F, M + 1], [F, M], [F, M] with 0 <= M <= 256."""
        every = (inst_idx, inst_off, best_box, best_cnt)
        dev = LpfContext._on_gpu("inside_masks", every, "list arrays")
        shp = [tuple(a.shape) for a in every]
        if any(len(t) != 2 for t in shp) or len({t[0] for t in shp}) != 1:
            raise ValueError("inside_masks: inst_idx [F, inst_cap], inst_off [F, M + 1], best_box [F, M], best_cnt [F, M], got %s" % (shp,))
        F, M = shp[0][0], shp[2][1]
        if shp[1][1] != M + 1 or shp[3][1] != M or not 0 <= M <= LPF_MAX_MASKS_WIDE:
            raise ValueError("inside_masks: inst_off [F, M + 1], best_box [F, M], best_cnt [F, M] with 0 <= M <= %d, got %s"
                             % (LPF_MAX_MASKS_WIDE, shp[1:]))
        if dev:
            names = [str(a.dtype).replace("torch.", "") for a in every]
            if names != ["int64", "int64", "int32", "int64"]:
                raise ValueError("inside_masks: GPU list arrays must be int64, int64, int32, int64, got %s" % names)
        return dev, F, M, shp[0][1]

    def inside_masks(self, frames, inst_idx, inst_off, best_box, best_cnt, min_points=10, want=INSIDE_WANT, out=None, staged=None):
        """V3's per-car inside / outside split of a batch of frames in ONE native call (lpf_inside_masks), from what a run on the same
        frames and boxes returned: ``inst_idx`` int64 [F, inst_cap], ``inst_off`` int64 [F, M + 1], ``best_box`` int32 [F, M],
        ``best_cnt`` int64 [F, M] -- all host arrays or all GPU tensors.  frames: as run_batch's (or ``staged=stage_points(frames)``).
        The boxes are the ones in force.  ``want`` picks the outputs (INSIDE_WANT): "inside" uint8 [F, inst_cap] parallel to inst_idx,
        "part_idx" int64 [F, inst_cap] and "part_xyz" float32 [F, inst_cap, 3] (per car: the inside entries first, then the outside
        ones), "n_inside" int64 [F, M], "matched" int32 [F, M].  Returns a dict of them: NumPy arrays after one host wait, or GPU
        tensors in torch's stream order (the call only enqueues work).  Entries the call does not write (beyond a frame's lists, rows
        of a frame whose lists did not fit) are zero, or what ``out`` -- a dict of the caller's own arrays under the same names -- held."""
        want = self._want("inside_masks", want, self.INSIDE_WANT)
        if int(min_points) < 0:
            raise ValueError("inside_masks: min_points must not be negative")
        dev, F, M, cap = self.inside_batch(inst_idx, inst_off, best_box, best_cnt)
        off, pts_ptr, pts_dev, _keep = staged or self._stage_points(frames)      # (_keep: alive until the call returns)
        if len(off) - 1 != F:
            raise ValueError("inside_masks: lists of %d frames, points of %d" % (F, len(off) - 1))
        lists = (inst_idx, inst_off, best_box, best_cnt)
        arrs = ([a.contiguous() for a in lists] if dev else
                [np.ascontiguousarray(a, dtype=t) for a, t in zip(lists, (np.int64, np.int64, np.int32, np.int64))])
        device = inst_idx.device if dev else None
        inp, o = InsideInput(), InsideOutputs()
        res = self._outputs("inside_masks", o, want, self._INSIDE_OUT, dict(F=F, cap=cap, M=M), device, out)
        inp.inst_idx, inp.inst_off, inp.best_box, inp.best_cnt = (_ptr(a) for a in arrs)
        inp.inst_cap, inp.M, inp.min_points, inp.on_device = cap, M, int(min_points), o.on_device
        if F:
            self._call_in_order(device, self._lib.lpf_inside_masks, pts_ptr, off.ctypes.data, F, pts_dev, ctypes.byref(inp), ctypes.byref(o))
        return res

    BOX_POINTS_WANT = ("box_points", "box_labelled", "first_box", "frame_counts")
    _BOX_POINTS_OUT = {"box_points": ("int32", ("B",), 0), "box_labelled": ("int32", ("B",), 0), "first_box": ("int32", ("N",), -1),
                       "frame_counts": ("int64", ("F", 4), 0)}

    @staticmethod
    def box_points_batch(valid_idx, n_valid, label_valid, Ntot, F):
        """The list arrays of box_points checked against a batch of F frames and Ntot points: (on_device, LW).  ValueError for host
        arrays mixed with GPU tensors, shapes that are not [Ntot], [F] and [Ntot] or [Ntot, LW] with 1 <= LW <= 8, and GPU tensors
        of another dtype than int64, int64 and int32 / uint32."""
        every = [a for a in (valid_idx, n_valid, label_valid) if a is not None]
        dev = LpfContext._on_gpu("box_points", every, "list arrays")
        shp = [tuple(a.shape) for a in (valid_idx, n_valid)]
        if shp[0] != (Ntot,) or shp[1] != (F,):
            raise ValueError("box_points: valid_idx [Ntot] and n_valid [F] of %d points in %d frames, got %s" % (Ntot, F, shp))
        LW = 0
        if label_valid is not None:
            ls = tuple(label_valid.shape)
            LW = 1 if len(ls) == 1 else (ls[1] if len(ls) == 2 else -1)
            if ls[:1] != (Ntot,) or not 1 <= LW <= LPF_MAX_MASKS_WIDE // 32:
                raise ValueError("box_points: label_valid [Ntot] or [Ntot, LW] with 1 <= LW <= %d for %d points, got %s"
                                 % (LPF_MAX_MASKS_WIDE // 32, Ntot, ls))
        if dev:
            names = [str(a.dtype).replace("torch.", "") for a in every]
            if names[:2] != ["int64", "int64"] or (len(names) == 3 and names[2] not in ("int32", "uint32")):
                raise ValueError("box_points: GPU list arrays must be int64, int64 and int32 / uint32, got %s" % names)
        return dev, LW

    def box_points(self, frames, valid_idx, n_valid, label_valid=None, want=BOX_POINTS_WANT, out=None, staged=None):
        """Per-box LiDAR point counts, the first box of every valid point and the point-level confusion counts of a batch of frames
        in ONE native call (lpf_box_points), from what a run on the same frames returned: ``valid_idx`` int64 [Ntot] (frame f's
        entries from the frame's first point on, as the runs write it), ``n_valid`` int64 [F] and ``label_valid`` uint32 [Ntot]
        (run_batch) or [Ntot, LW] (run_wide), or None: nothing is labelled -- all host arrays or all GPU tensors.  frames: as
        run_batch's (or ``staged=stage_points(frames)``).  The boxes are the ones in force.  ``want`` picks the outputs
        (BOX_POINTS_WANT): "box_points" and "box_labelled" int32 [Btot], "first_box" int32 [Ntot] parallel to valid_idx (-1: in no
        box), "frame_counts" int64 [F, 4] = {valid, in a box, labelled, labelled and in a box}.  Returns a dict of them: NumPy arrays
        after one host wait, or GPU tensors in torch's stream order (the call only enqueues work).  Entries of first_box the call
        does not write (beyond a frame's n_valid) are -1, or what ``out`` -- a dict of the caller's own arrays under the same names
        -- held."""
        want = self._want("box_points", want, self.BOX_POINTS_WANT)
        off, pts_ptr, pts_dev, _keep = staged or self._stage_points(frames)      # (_keep: alive until the call returns)
        F, Ntot = len(off) - 1, int(off[-1])
        dev, LW = self.box_points_batch(valid_idx, n_valid, label_valid, Ntot, F)
        if self.box_off is None or len(self.box_off) - 1 != F:
            raise ValueError("box_points: boxes in force for %s frames, points of %d (set_boxes* comes first)"
                             % ("no" if self.box_off is None else len(self.box_off) - 1, F))
        device = valid_idx.device if dev else None
        if dev:
            import torch
            arrs = [None if a is None else a.contiguous() for a in (valid_idx, n_valid, label_valid)]
        else:
            arrs = [None if a is None else np.ascontiguousarray(a, dtype=t)
                    for a, t in zip((valid_idx, n_valid, label_valid), (np.int64, np.int64, np.uint32))]
        if Ntot == 0:                                      # (an empty array has no address, and the call wants one)
            arrs[0] = torch.zeros(1, dtype=torch.int64, device=device) if dev else np.zeros(1, np.int64)
        inp, o = BoxPointsInput(), BoxPointsOutputs()
        res = self._outputs("box_points", o, want, self._BOX_POINTS_OUT, dict(B=int(self.box_off[-1]), N=Ntot, F=F), device, out)
        inp.valid_idx, inp.n_valid, inp.label_valid_words = (_ptr(a) for a in arrs)
        inp.LW, inp.on_device = LW, o.on_device
        if F:
            self._call_in_order(device, self._lib.lpf_box_points, pts_ptr, off.ctypes.data, F, pts_dev, ctypes.byref(inp), ctypes.byref(o))
        return res

    _FIRST_MATCH_OUT = {"first_mask": ("int32", ("N",), -2), "car_idx": ("int64", ("N",), -1), "car_mask": ("int32", ("N",), -1),
                        "car_xyz": ("float32", ("N", 3), 0), "car_rgb": ("float64", ("N", 3), 0), "bg_idx": ("int64", ("N",), -1),
                        "bg_xyz": ("float32", ("N", 3), 0), "n_valid": ("int64", ("F",), 0), "n_car": ("int64", ("F",), 0),
                        "n_bg": ("int64", ("F",), 0), "mask_count": ("int64", ("F", "M"), 0)}
    FIRST_MATCH_WANT = tuple(_FIRST_MATCH_OUT)
    _FIRST_MATCH_LISTS = ("car_idx", "car_mask", "car_xyz", "car_rgb", "bg_idx", "bg_xyz")

    @staticmethod
    def first_match_batch(masks, colors, F):
        """The masks [F,M,mh,mw] (or [M,mh,mw] for one frame) and colours [F,M,3] (or [M,3]; None: none) of first_match checked against
        a batch of F frames: (on_device, M, mh, mw, f32, masks, colors) with the two arrays contiguous, uint8 or float32 and float64.
        ValueError for other shapes, more than LPF_MAX_MASKS_WIDE masks, an empty plane with M > 0, host arrays mixed with GPU tensors
        and GPU tensors of another dtype than uint8 / bool / float32 and float64."""
        dev = LpfContext._on_gpu("first_match", [a for a in (masks, colors) if a is not None], "arrays")
        if not dev:
            masks = np.asarray(masks)
        shp = tuple(masks.shape)
        if len(shp) == 3 and F == 1:
            masks, shp = masks[None], (1,) + shp
        if len(shp) != 4 or shp[0] != F:
            raise ValueError("first_match: masks [F,M,mh,mw] for %d frames (or [M,mh,mw] for one), got %s" % (F, shp))
        M, mh, mw = (int(x) for x in shp[1:])
        if M > LPF_MAX_MASKS_WIDE:
            raise ValueError("first_match: %d masks per frame, one call takes %d" % (M, LPF_MAX_MASKS_WIDE))
        if M > 0 and (mh < 1 or mw < 1):
            raise ValueError("first_match: masks of %d x %d pixels" % (mh, mw))
        name = str(masks.dtype).replace("torch.", "")
        f32 = name not in ("uint8", "bool")
        if dev:
            import torch
            if name not in ("uint8", "bool", "float32"):
                raise ValueError("first_match: GPU masks must be uint8, bool or float32, got %s" % name)
            masks = (masks.to(torch.uint8) if name == "bool" else masks).contiguous()
        else:
            if masks.dtype.kind not in "buif":
                raise ValueError("first_match: masks must be uint8, bool or float, got %s" % name)
            masks = np.ascontiguousarray(masks, dtype=np.float32 if f32 else np.uint8)
        return dev, M, mh, mw, int(f32), masks, LpfContext._first_match_colors(colors, F, M, dev)

    @staticmethod
    def _first_match_colors(colors, F, M, dev):
        """first_match's colours [F,M,3] (or [M,3] for one frame; None: none), contiguous float64: a host array (any numbers), or with
        ``dev`` a GPU tensor, which must be float64."""
        if colors is None:
            return None
        if not dev:
            colors = np.ascontiguousarray(colors, dtype=np.float64)
        cs = tuple(colors.shape)
        if len(cs) == 2 and F == 1:
            colors, cs = colors[None], (1,) + cs
        if cs != (F, M, 3):
            raise ValueError("first_match: colors [F,M,3] = %s, got %s" % ((F, M, 3), cs))
        if dev:
            if str(colors.dtype) != "torch.float64":
                raise ValueError("first_match: GPU colors must be float64, got %s" % colors.dtype)
            colors = colors.contiguous()
        return colors

    @staticmethod
    def first_match_rle_batch(masks, colors, F, out=None):
        """first_match's masks in run-length form -- one rle.RleMasks (F = 1), or a list with one per frame -- checked against a batch of
        F frames before any native call: ``(device, M, mh, mw, (runs, run_off, RleMasksInput), colors)``; None when ``masks`` are not in
        that form.  The frames share one size, which becomes mh x mw (it need not be the camera's); ragged M is padded with empty
        masks, up to LPF_MAX_MASKS_WIDE.  The masks stay host memory; device: where the outputs go -- the GPU of ``out``'s tensors or
        of GPU ``colors``, else None (NumPy).  ValueError: a list that mixes RleMasks and arrays, frames of differing sizes, more than
        256 masks, another frame count, colours of another shape or dtype."""
        found = compact_frames(masks, "first_match", ("rle",))
        if found is None:
            return None
        frames = found[1]
        if len(frames) != F:
            raise ValueError("first_match: RleMasks for %d frames, the batch has %d" % (len(frames), F))
        sizes = sorted({tuple(r.shape[1:]) for r in frames})
        if len(sizes) > 1:
            raise ValueError("first_match: the frames' RleMasks have differing sizes (H, W) = %s: one size per call (runs are not resized)"
                             % (sizes,))
        mh, mw = sizes[0] if sizes else (1, 1)
        runs, run_off, _, M = LpfContext.rle_batch(frames, mh, mw, LPF_MAX_MASKS_WIDE, "first_match")
        on_gpu = _is_torch(colors) and colors.is_cuda
        device = colors.device if on_gpu else None
        colors = LpfContext._first_match_colors(colors, F, M, on_gpu)
        for t in (out or {}).values():
            if _is_torch(t) and t.is_cuda:
                device = t.device
        return device, M, int(mh), int(mw), (runs, run_off, RleMasksInput.of(runs, run_off, F, M)), colors

    def first_match(self, pts_per_frame, masks, colors=None, want=None, out=None, staged=None, rects=None, binarize=None, erode_iters=0):
        """Same_color.py:113-132's exclusive labels of a batch of frames in ONE native call (lpf_first_match): every valid point goes
        to the FIRST mask of its frame with ``v < mh and u < mw and mask[v, u] > 0.5`` (uint8 / bool masks: nonzero), or to the
        background.  pts_per_frame: as run_batch's frames -- f32 [N_f,4] host arrays, Scans of a ScanReader, float32 [N,4] GPU tensors
        (or ``staged=stage_points(frames)``).  masks: [F,M,mh,mw] (or [M,mh,mw] for one frame) at the masks' OWN size, which need not
        be the camera's; colors: float64 [F,M,3], the rows "car_rgb" gathers -- both host arrays or both GPU tensors.  The camera,
        transform and depth window are set_camera's.  ``want`` picks the outputs (FIRST_MATCH_WANT; "n_car" and "n_bg" always come;
        None: all of them, "car_rgb" when there are colors):
        "first_mask" int32 [Ntot] (-2 not valid, -1 background, else the mask), the compact lists "car_idx" int64 / "car_mask" int32 /
        "car_xyz" float32 [.,3] / "car_rgb" float64 [.,3] / "bg_idx" / "bg_xyz" -- frame f's entries from the frame's first point on,
        n_car[f] resp. n_bg[f] of them, ascending -- and "n_valid", "n_car", "n_bg" int64 [F], "mask_count" int64 [F,M].  Returns a dict
        of them plus "frame_off": NumPy arrays after one host wait, or GPU tensors in torch's stream order when the masks are GPU
        tensors (the call only enqueues work).  Entries the call does not write (beyond a frame's count) are -1 / 0, or what ``out``
        -- a dict of the caller's own arrays under the same names -- held.
        masks in run-length form -- one rle.RleMasks (one frame), or a list with one per frame, all of ONE size, which is mh x mw
        (ragged M is padded with empty masks) -- go through lpf_first_match_rle: the runs are decoded into label planes on the GPU,
        nothing dense crosses to the device, and every result equals the one ``.to_dense()`` masks give.  They stay host memory; the
        outputs are GPU tensors when ``out`` holds GPU tensors or ``colors`` is one.  The labelling has no rectangles, no binarize
        rule of its own ("gt0.5" is the rule) and no erosion: ``rects``, another ``binarize`` and ``erode_iters`` are ValueErrors."""
        if rects is not None or binarize not in (None, "gt0.5") or erode_iters != 0:
            raise ValueError("first_match: rects=%s binarize=%r erode_iters=%r: the first-mask labelling takes no rectangles, reads masks "
                             "as > 0.5 / nonzero and has no erosion" % ("given" if rects is not None else None, binarize, erode_iters))
        if want is None:
            want = tuple(w for w in self.FIRST_MATCH_WANT if w != "car_rgb" or colors is not None)
        want = self._want("first_match", want, self.FIRST_MATCH_WANT)
        want = want + tuple(w for w in ("n_car", "n_bg") if w not in want)
        if "car_rgb" in want and colors is None:
            raise ValueError("first_match: car_rgb is wanted, colors is None")
        off, pts_ptr, pts_dev, _keep = staged or self._stage_points(pts_per_frame)      # (_keep: alive until the call returns)
        F, Ntot = len(off) - 1, int(off[-1])
        # the two forms differ in the input struct, the native function, where the outputs go and what must outlive the call
        rle = self.first_match_rle_batch(masks, colors, F, out)
        if rle is not None:
            device, M, mh, mw, tables, colors = rle
            native, inp = "lpf_first_match_rle", FirstMatchRleInput()
            inp.masks = ctypes.pointer(tables[2])
            inp.colors_on_device = int(_is_torch(colors))
            lend = [(_keep, tables, colors)] if device is not None else []      # (staged points, tables and colours: alive until the work has run)
        else:
            dev, M, mh, mw, f32, masks, colors = self.first_match_batch(masks, colors, F)
            device = masks.device if dev else None
            native, inp = "lpf_first_match", FirstMatchInput()
            inp.masks = _ptr(masks) if M else None
            inp.M, inp.f32, inp.on_device = M, f32, int(dev)
            lend = []
        o = FirstMatchOutputs()
        res = self._outputs("first_match", o, want, self._FIRST_MATCH_OUT, dict(N=Ntot, F=F, M=M), device, out)
        if Ntot == 0:                                       # (an empty array has no address: nothing would be written to it)
            for w in self._FIRST_MATCH_LISTS + ("first_mask",):
                setattr(o, w, None)
        inp.mh, inp.mw = mh, mw
        inp.colors = _ptr(colors) if (colors is not None and M) else None
        if inp.colors is None:
            o.car_rgb = None                                # (no mask, no car point: nothing to gather)
        if F:
            self._call_in_order(device, getattr(self._lib, native), pts_ptr, off.ctypes.data, F, pts_dev, ctypes.byref(inp), ctypes.byref(o))
            self._lent.extend(lend)
        res["frame_off"] = off
        return res

    _BOX_VIEWS_OUT = {"keep": ("uint8", ("B",), 0), "reason": ("int32", ("B",), 0), "corners_in_view": ("int32", ("B",), 0),
                      "corners_near": ("int32", ("B",), 0), "avg_depth": ("float64", ("B",), 0), "near_bbox2d": ("float64", ("B", 4), 0),
                      "front": ("int32", ("B",), 0), "bbox2d": ("float64", ("B", 4), 0), "front_avg_depth": ("float64", ("B",), 0),
                      "kept_pos": ("int32", ("B",), 0), "frame_counts": ("int32", ("F", 6), 0), "corners_velo": ("float64", ("B", 8, 3), 0)}
    BOX_VIEWS_WANT = tuple(_BOX_VIEWS_OUT)
    BOX_VIEW_REASONS = ("valid", "no_corners", "all_behind_camera", "no_intersection", "too_small", "error")

    @classmethod
    def box_views_batch(cls, corners, box_off, T_cam_to_velo=None, min_points_in_view=4, depth_range=(0.1, 100), min_area=100,
                        want=("keep", "reason")):
        """The arguments of box_views checked and described: (on_device, box_off int32 [F+1], want tuple).  ValueError for corners
        that are not float64 [Btot,8,3] (any numbers for host arrays), a box_off that is not [F+1] from 0 to Btot without a decrease,
        an unknown or empty ``want``, "corners_velo" without T_cam_to_velo, thresholds that are not finite and min_points_in_view
        outside 0..8."""
        want = cls._want("box_views", want, cls.BOX_VIEWS_WANT)
        dev = _is_torch(corners) and bool(corners.is_cuda)
        if _is_torch(corners) and not dev:
            corners = corners.numpy()
        if not dev:
            corners = np.asarray(corners)
            if corners.dtype.kind not in "fiu":
                raise ValueError("box_views: corners must be numbers, got %s" % corners.dtype)
        elif str(corners.dtype) != "torch.float64":
            raise ValueError("box_views: GPU corners must be float64, got %s" % corners.dtype)
        shape = tuple(corners.shape)
        if len(shape) != 3 or shape[1:] != (8, 3):
            raise ValueError("box_views: corners must be [Btot,8,3] (cam-0 corners), got %s" % (shape,))
        off = np.asarray(box_off)
        if off.ndim != 1 or len(off) < 1 or off.dtype.kind not in "iu":
            raise ValueError("box_views: box_off must be integers [F+1], got %s %s" % (off.dtype, off.shape))
        off = off.astype(np.int64)
        if off[0] != 0 or off[-1] != shape[0] or (np.diff(off) < 0).any():
            raise ValueError("box_views: box_off must rise from 0 to the %d boxes without a decrease, got %s .. %s"
                             % (shape[0], off[0], off[-1]))
        if shape[0] > 0x7fffffff:
            raise ValueError("box_views: %d boxes, a call takes fewer than 2^31" % shape[0])
        if "corners_velo" in want and T_cam_to_velo is None:
            raise ValueError("box_views: \"corners_velo\" needs T_cam_to_velo")
        if T_cam_to_velo is not None and np.asarray(T_cam_to_velo).size != 16:
            raise ValueError("box_views: T_cam_to_velo must be 4 x 4, got %s" % (np.asarray(T_cam_to_velo).shape,))
        try:
            lo, hi = (float(v) for v in depth_range)
            nums = (lo, hi, float(min_area))
        except (TypeError, ValueError):
            raise ValueError("box_views: depth_range is (lo, hi) and min_area a number") from None
        if not all(np.isfinite(nums)):
            raise ValueError("box_views: depth_range and min_area must be finite numbers, got %s" % (nums,))
        if int(min_points_in_view) != min_points_in_view or not 0 <= int(min_points_in_view) <= 8:
            raise ValueError("box_views: min_points_in_view must be an integer in 0..8, got %r" % (min_points_in_view,))
        return dev, off.astype(np.int32), want

    def box_views(self, corners, box_off, T_cam_to_velo=None, min_points_in_view=4, depth_range=(0.1, 100), min_area=100,
                  want=("keep", "reason")):
        """secondtest.py's camera-view filter (is_bbox_in_camera_view) and V5's detailed box projection (project_3d_bbox_to_2d) for
        every box of a batch of frames in ONE native call (lpf_box_views; needs set_camera / ensure_intrinsics first).  ``corners``:
        float64 [Btot,8,3] cam-0 corners, a NumPy array or a GPU tensor; ``box_off`` int [F+1]: frame f owns boxes box_off[f] ..
        box_off[f+1].  ``want`` picks the outputs (BOX_VIEWS_WANT): "keep" uint8, "reason" int32 (an index into BOX_VIEW_REASONS),
        "corners_in_view", "corners_near", "front", "kept_pos" int32 [Btot], "avg_depth", "front_avg_depth" float64 [Btot],
        "near_bbox2d", "bbox2d" float64 [Btot,4] ({min u, min v, max u, max v}; bbox2d / front as prepare_boxes returns them),
        "frame_counts" int32 [F,6] (boxes per reason, [0] = kept), "corners_velo" float64 [Btot,8,3] (needs T_cam_to_velo).  Returns a
        dict of them: NumPy arrays after one host wait, or GPU tensors on the corners' device in torch's stream order (the call only
        enqueues work).  The arithmetic is the reference's, statement for statement (include/lpf.h)."""
        dev, off, want = self.box_views_batch(corners, box_off, T_cam_to_velo, min_points_in_view, depth_range, min_area, want)
        F, Btot = len(off) - 1, int(off[-1])
        device = corners.device if dev else None
        cc = corners.contiguous() if dev else np.ascontiguousarray(corners.numpy() if _is_torch(corners) else corners, dtype=np.float64)
        inp, o = BoxViewsInput(), BoxViewsOutputs()
        res = self._outputs("box_views", o, want, self._BOX_VIEWS_OUT, dict(B=Btot, F=F), device)
        T = None if T_cam_to_velo is None else np.ascontiguousarray(T_cam_to_velo, dtype=np.float64).reshape(16)
        inp.corners_cam0, inp.box_off, inp.T_cam_to_velo, inp.on_device = _ptr(cc), off.ctypes.data, _ptr(T), o.on_device
        inp.min_points_in_view = int(min_points_in_view)
        inp.depth_lo, inp.depth_hi, inp.min_area = float(depth_range[0]), float(depth_range[1]), float(min_area)
        if F:
            self._call_in_order(device, self._lib.lpf_box_views, F, ctypes.byref(inp), ctypes.byref(o))
        return res

    def run_cams_wide(self, frames, cams, want_uv=True, want_float=False, want_lists=True, want_valid_uv=False, inst_cap=None,
                      want_label=True, pinned=False):
        """run_cams with up to 256 masks per camera, in ONE native pass (lpf_run_cams_wide): the points are staged once (as run_batch's
        ``frames``) and read once by the GPU, every camera's masks give ceil(M / 32) label words per point.  cams: run_cams' camera
        dicts, masks of up to 256 per frame.  Returns ``results[c][f]``: what run_wide returns for frame f after set_camera / set_boxes
        with camera c's arguments -- equal, array for array.  The context's camera, masks and boxes are left as they were.
        want_label=False leaves out the dense label_words (label_valid_words, with want_valid_uv, still come back).  pinned=True: the
        result arrays are views into page-locked buffers the context owns and reuses -- valid until the next run on this context."""
        cin, Ms, box_offs, _keep_in = self._cam_inputs(frames, cams, LPF_MAX_MASKS_WIDE, "run_cams_wide")
        C, F = len(cams), len(frames)
        off, pts_ptr, pts_dev, _keep = self._stage_points(frames)      # (_keep: alive until the run returns)
        n = int(off[-1])
        wants = dict(want_uv=want_uv, want_float=want_float, want_lists=want_lists, want_valid_uv=want_valid_uv, want_label=want_label,
                     pinned=pinned)

        def launch(inst_cap):
            outs = (WideOutputs * C)()
            fins = [self._wide_host_outputs(outs[k], n, F, Ms[k], int(box_offs[k][-1]) if box_offs[k] is not None else 0, inst_cap,
                                            tag="cam%d_" % k, **wants) for k in range(C)]
            self._check(self._lib.lpf_run_cams_wide(self._h, pts_ptr, off.ctypes.data, F, pts_dev, cin, C, outs))
            res = [fin() for fin in fins]
            return [r for r, _ in res], max(need for _, need in res)

        outs = self._until_lists_fit(launch, inst_cap, off)
        return [self._frame_results(off, Ms[k], *outs[k], box_off=box_offs[k]) for k in range(C)]

    # -- the hot path, device tensors (asynchronous) -------------------------------------
    def run_device(self, pts, frame_off, uv=None, label_bits=None, depth=None, u_f=None, v_f=None,
                   valid_idx=None, inst_idx=None, inst_cap=0, count_mb=None, summary=None, uv_valid=None, label_valid=None):
        """Enqueue one batch on the context's stream.  pts: torch float32 [Ntot,4] on the GPU;
        outputs: preallocated torch tensors (None = not wanted); summary: uint8 [F*928].
        frame_off: int64 NumPy/sequence [F+1] (host)."""
        off = np.ascontiguousarray(frame_off, dtype=np.int64)
        F = off.shape[0] - 1
        o = Outputs()
        o.on_device = 1
        o.uv = _dev_ptr(uv, "int32")
        o.label_bits = _dev_ptr(label_bits)
        o.depth, o.u_f, o.v_f = _dev_ptr(depth, "float64"), _dev_ptr(u_f, "float64"), _dev_ptr(v_f, "float64")
        o.valid_idx = _dev_ptr(valid_idx, "int64")
        o.inst_idx = _dev_ptr(inst_idx, "int64")
        o.inst_cap = int(inst_cap)
        o.count_mb = _dev_ptr(count_mb, "int32")
        o.summary = _dev_ptr(summary)
        o.uv_valid, o.label_valid = _dev_ptr(uv_valid, "int32"), _dev_ptr(label_valid)
        self._check(self._lib.lpf_run_batch(self._h, _dev_ptr(pts, "float32"), off.ctypes.data, F, 1,
                                            ctypes.byref(o)))

    def make_frame_step(self, pts, masks_u8=None, mask_rects=None, boxes_cam0=None, T_cam_to_velo=None, filter_visible=True, oriented=True, **outs):
        """Pre-marshal ONE frame of a stream -- scan, lent uint8 masks [M,H,W] (+ their rectangles [M,4]), lent cam-0 box corners
        [B,8,3], output tensors as in make_device_step -- into an lpf_frame_job and return a zero-argument callable that makes the one
        C call (lpf_run_frame): masks, rectangles, boxes and the run in a single FFI crossing.  Lent tensors stay unchanged until the
        frame's results are complete (pipelined modes: two launches later)."""
        j = FrameJob()
        n = int(pts.shape[0])
        j.pts, j.n_points = _dev_ptr(pts, "float32"), n
        keep = [pts, outs]
        if masks_u8 is not None:
            shape = tuple(masks_u8.shape)
            if len(shape) != 3 or shape[1:] != (self.H, self.W) or str(masks_u8.dtype) != "torch.uint8":
                raise ValueError("masks_u8 must be a torch.uint8 GPU tensor [M,H,W]")
            j.masks, j.n_masks = _dev_ptr(masks_u8), shape[0]
            self.F_masks, self.M = 1, shape[0]
            keep.append(masks_u8)
            if mask_rects is not None:
                if tuple(mask_rects.shape) != (shape[0], 4) or str(mask_rects.dtype) != "torch.int32" or not mask_rects.is_contiguous():
                    raise ValueError("mask_rects must be a contiguous torch.int32 GPU tensor [M,4]")
                j.mask_rects = _dev_ptr(mask_rects)
                keep.append(mask_rects)
        if boxes_cam0 is not None:
            Tcv = np.ascontiguousarray(T_cam_to_velo, dtype=np.float64).reshape(16)
            j.corners_cam0, j.n_boxes, j.T_cam_to_velo = _dev_ptr(boxes_cam0, "float64") if boxes_cam0.shape[0] else None, int(boxes_cam0.shape[0]), Tcv.ctypes.data
            j.filter_visible, j.oriented = int(bool(filter_visible)), int(bool(oriented))
            self.box_off = np.array([0, int(boxes_cam0.shape[0])], np.int32)
            keep += [boxes_cam0, Tcv]
        o = j.out
        o.on_device = 1
        o.uv = _dev_ptr(outs.get("uv"), "int32")
        o.label_bits = _dev_ptr(outs.get("label_bits"))
        o.depth, o.u_f, o.v_f = (_dev_ptr(outs.get("depth"), "float64"), _dev_ptr(outs.get("u_f"), "float64"), _dev_ptr(outs.get("v_f"), "float64"))
        o.valid_idx = _dev_ptr(outs.get("valid_idx"), "int64")
        o.inst_idx = _dev_ptr(outs.get("inst_idx"), "int64")
        o.inst_cap = int(outs.get("inst_cap", 0))
        o.count_mb = _dev_ptr(outs.get("count_mb"), "int32")
        o.summary = _dev_ptr(outs.get("summary"))
        o.uv_valid, o.label_valid = _dev_ptr(outs.get("uv_valid"), "int32"), _dev_ptr(outs.get("label_valid"))
        run, h, check, ref = self._lib.lpf_run_frame, self._h, self._check, ctypes.byref(j)

        def fn(_keep=(j, keep)):
            rc = run(h, ref)
            if rc:
                check(rc)
        return fn

    _WIDE_OUTS = {"uv": "int32", "depth": "float64", "u_f": "float64", "v_f": "float64", "valid_idx": "int64", "uv_valid": "int32",
                  "label_words": None, "label_valid_words": None, "inst_idx": "int64", "count_mb": "int32", "n_valid": "int64",
                  "n_labelled": "int64", "inst_count": "int64", "inst_off": "int64", "best_cnt": "int64", "best_box": "int32",
                  "inst_overflow": "int32"}

    def make_frame_step_wide(self, pts, masks_u8, mask_rects=None, boxes_cam0=None, T_cam_to_velo=None, filter_visible=True, oriented=True,
                             **outs):
        """make_frame_step for frames with up to 256 masks: pre-marshal ONE frame -- scan, lent uint8 masks [M,H,W] (+ their rectangles
        [M,4]), lent cam-0 box corners [B,8,3] -- into an lpf_frame_job_wide and return a zero-argument callable that makes the one C
        call (lpf_run_frame_wide).  outs: GPU tensors named after the lpf_wide_outputs fields (uv, depth, u_f, v_f, valid_idx, uv_valid,
        label_words [N, ceil(M/32)], label_valid_words, inst_idx, count_mb, n_valid, n_labelled, inst_count, inst_off, best_cnt,
        best_box, inst_overflow), plus inst_cap.  Lent tensors stay unchanged until the frame's results are complete."""
        bad = set(outs) - set(self._WIDE_OUTS) - {"inst_cap"}
        if bad:
            raise ValueError("unknown outputs %s" % sorted(bad))
        def tensor(t):
            return _is_torch(t) and hasattr(t, "is_cuda")

        # shapes and dtypes first, then where the tensors live: nothing reaches the native library before every check has passed
        if not tensor(pts) or str(pts.dtype) != "torch.float32" or pts.dim() != 2 or pts.shape[1] != 4 or not pts.is_contiguous():
            raise ValueError("pts must be a contiguous torch.float32 tensor [N,4]")
        if not tensor(masks_u8) or str(masks_u8.dtype) != "torch.uint8" or masks_u8.dim() != 3 or not masks_u8.is_contiguous():
            raise ValueError("masks_u8 must be a contiguous torch.uint8 tensor [M,H,W]")
        M = int(masks_u8.shape[0])
        if M > LPF_MAX_MASKS_WIDE:
            raise ValueError("at most %d masks per frame, got %d" % (LPF_MAX_MASKS_WIDE, M))
        if tuple(masks_u8.shape[1:]) != (self.H, self.W):
            raise ValueError("masks_u8 must be [M,%d,%d] (the camera's size), got %s" % (self.H, self.W, tuple(masks_u8.shape)))
        if mask_rects is not None and (not tensor(mask_rects) or str(mask_rects.dtype) != "torch.int32" or tuple(mask_rects.shape) != (M, 4)
                                       or not mask_rects.is_contiguous()):
            raise ValueError("mask_rects must be a contiguous torch.int32 tensor [M=%d,4]" % M)
        if boxes_cam0 is not None and (not tensor(boxes_cam0) or str(boxes_cam0.dtype) != "torch.float64" or boxes_cam0.dim() != 3
                                       or tuple(boxes_cam0.shape[1:]) != (8, 3) or not boxes_cam0.is_contiguous()):
            raise ValueError("boxes_cam0 must be a contiguous torch.float64 tensor [B,8,3]")
        if boxes_cam0 is not None and np.asarray(T_cam_to_velo, dtype=np.float64).size != 16:
            raise ValueError("T_cam_to_velo must be a 4x4 matrix")
        for k, t in outs.items():
            if k != "inst_cap" and t is not None and (not tensor(t) or not t.is_contiguous()):
                raise ValueError("output %s must be a contiguous tensor" % k)
        for k, t in [("pts", pts), ("masks_u8", masks_u8), ("mask_rects", mask_rects), ("boxes_cam0", boxes_cam0)] + list(outs.items()):
            if k != "inst_cap" and t is not None and not t.is_cuda:
                raise ValueError("%s must be a GPU tensor: lpf_run_frame_wide takes device memory only" % k)
        j = FrameJobWide()
        j.pts, j.n_points = _dev_ptr(pts, "float32"), int(pts.shape[0])
        j.masks, j.n_masks = (_dev_ptr(masks_u8) if M else None), M
        j.mask_rects = _dev_ptr(mask_rects) if (mask_rects is not None and M) else None
        keep = [pts, masks_u8, mask_rects, outs]
        if boxes_cam0 is not None:
            Tcv = np.ascontiguousarray(T_cam_to_velo, dtype=np.float64).reshape(16)
            B = int(boxes_cam0.shape[0])
            j.corners_cam0, j.n_boxes, j.T_cam_to_velo = _dev_ptr(boxes_cam0, "float64") if B else None, B, Tcv.ctypes.data
            j.filter_visible, j.oriented = int(bool(filter_visible)), int(bool(oriented))
            self.box_off = np.array([0, B], np.int32)
            keep += [boxes_cam0, Tcv]
        o = j.out
        o.on_device = 1
        for k, dt in self._WIDE_OUTS.items():
            setattr(o, k, _dev_ptr(outs.get(k), dt))
        o.inst_cap = int(outs.get("inst_cap", 0))
        run, h, check, ref = self._lib.lpf_run_frame_wide, self._h, self._check, ctypes.byref(j)

        def fn(_keep=(j, keep)):
            rc = run(h, ref)
            if rc:
                check(rc)
        return fn

    def make_device_step(self, pts, frame_off, masks_u8=None, erode_iters=0, lend=False, boxes_cam0=None, box_off=None,
                         T_cam_to_velo=None, filter_visible=True, oriented=True, mask_rects=None, **outs):
        """Pre-marshal one device-mode step -- optional u8 masks, optional per-step boxes (the reference's per-frame box
        preparation from cam-0 corners, V3:556-562), run_batch -- and return a zero-argument callable that only performs the C
        calls: for launch-bound loops.
        lend=False: the mask tensor may be rewritten, in stream order, right after the step call returns (it is packed by a
        launch of its own at the call).  lend=True passes masks (and box corners) as LENT (on_device = 2): nothing is copied or
        packed at the call -- in the "fused-pack" mode the pack and the box set-up ride in the step's launch, small sparse launches
        read the masks directly -- but the tensors must then stay UNCHANGED until the step's results are complete (in the
        pipelined modes a step's inputs are read up to two launches later).
        mask_rects: int32 torch GPU tensor [F,M,4], the masks' rectangles (set_mask_rects), lent like the masks."""
        off = np.ascontiguousarray(frame_off, dtype=np.int64)
        F = off.shape[0] - 1
        o = Outputs()
        o.on_device = 1
        o.uv = _dev_ptr(outs.get("uv"), "int32")
        o.label_bits = _dev_ptr(outs.get("label_bits"))
        o.depth, o.u_f, o.v_f = (_dev_ptr(outs.get("depth"), "float64"), _dev_ptr(outs.get("u_f"), "float64"),
                                 _dev_ptr(outs.get("v_f"), "float64"))
        o.valid_idx = _dev_ptr(outs.get("valid_idx"), "int64")
        o.inst_idx = _dev_ptr(outs.get("inst_idx"), "int64")
        o.inst_cap = int(outs.get("inst_cap", 0))
        o.count_mb = _dev_ptr(outs.get("count_mb"), "int32")
        o.summary = _dev_ptr(outs.get("summary"))
        o.uv_valid, o.label_valid = _dev_ptr(outs.get("uv_valid"), "int32"), _dev_ptr(outs.get("label_valid"))
        lib, h, check = self._lib, self._h, self._check
        p_pts, p_off, p_out = _P(_dev_ptr(pts, "float32")), _P(off.ctypes.data), ctypes.byref(o)
        run, setm, setb = lib.lpf_run_batch, lib.lpf_set_masks_u8, lib.lpf_set_boxes_cam0
        where = 2 if lend else 1
        calls = []
        keep = [off, o, pts, outs]
        if masks_u8 is not None:
            shape = tuple(masks_u8.shape)
            if len(shape) == 3:
                shape = (1,) + shape
            if shape[0] != F or shape[2:] != (self.H, self.W) or str(masks_u8.dtype) != "torch.uint8":
                raise ValueError("masks_u8 must be a torch.uint8 GPU tensor [F,M,H,W]")
            p_m, M, it = _P(_dev_ptr(masks_u8)), shape[1], int(erode_iters)
            self.F_masks, self.M = F, M
            keep.append(masks_u8)
            if mask_rects is not None:
                if tuple(mask_rects.shape) != (F, M, 4) or str(mask_rects.dtype) != "torch.int32" or not mask_rects.is_contiguous():
                    raise ValueError("mask_rects must be a contiguous torch.int32 GPU tensor [F,M,4]")
                p_r, setr = _P(_dev_ptr(mask_rects)), lib.lpf_set_mask_rects
                keep.append(mask_rects)
                calls.append(lambda: setr(h, p_r, 1, F, M))
            calls.append(lambda: setm(h, p_m, F, M, it, where))
        if boxes_cam0 is not None:
            boff = np.ascontiguousarray(box_off, dtype=np.int32)
            if boff.shape[0] != F + 1:
                raise ValueError("box_off must have F + 1 entries")
            Tcv = np.ascontiguousarray(T_cam_to_velo, dtype=np.float64).reshape(16)
            p_b = _P(_dev_ptr(boxes_cam0, "float64")) if int(boff[-1]) else None
            p_bo, p_T, fv, ori = _P(boff.ctypes.data), _P(Tcv.ctypes.data), int(bool(filter_visible)), int(bool(oriented))
            self.box_off = boff
            keep += [boxes_cam0, boff, Tcv]
            calls.append(lambda: setb(h, p_b, where, p_bo, F, p_T, fv, ori, None, None, None, None))
        calls.append(lambda: run(h, p_pts, p_off, F, 1, p_out))
        calls = tuple(calls)

        def fn(_keep=tuple(keep)):
            for call in calls:
                rc = call()
                if rc:
                    check(rc)
        return fn
