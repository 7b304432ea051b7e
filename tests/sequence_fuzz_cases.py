"""Draws, state model and checker of the model-based SEQUENCE fuzz: a seed draws 10 to 14 calls on ONE long-lived LpfContext, a small
model carries the state include/lpf.h documents (camera, masks, boxes in force, erosion element, pipelined mode, work owed), and every
call's outputs are compared, bit for bit, with the reference for the state the model says is in force.  tests/test_gpu_sequence_fuzz.py
runs the sequences on the GPU; tests/test_sequence_fuzz_cases.py proves on the CPU, from the model and the references alone, what the
default seeds reach and that the checker notices one wrong entry and one overwritten poison byte.  Not a test module.

The ops are built from the existing generators and references, not copies of them: narrow_fuzz_cases.case (with the camera size, mask
count, element and frame sizes chosen here), wide_fuzz_cases._draw_camera / oracle_result / reference, batch_range_cases' batches of
lpf_match_2d, lpf_assign_costs and lpf_assign_2d, first_match_ref, box_views_ref, erosion_ref and test_gpu_depth_maps._expect.

Op kinds (FAMILIES):
  narrow        a narrow case: set_camera, the masks from their source (host, device, lent, lent and unaligned, a label image), their
                rectangles, the boxes from their source, then run_device (device outputs, poisoned), run_batch (host outputs; in
                order only: under a pipelined mode the op takes the device route) or make_frame_step (one frame, lent uint8 masks)
  rerun         the last narrow run again with fresh outputs and NOTHING set again that the header lets stand: in order no set-up
                call at all; in a pipelined mode, or after a mode switch, the masks again (with the element now in force); the boxes
                never.  After a frame step, in order, a step with NULL masks and NULL corners.
  rerun-unset   the rerun WITHOUT its masks: in order a plain rerun; in a pipelined mode with masks the documented refusal
                (REFUSAL), after which the next op has to be right
  wide          run_wide with NULL corners on the last run's frames: the model's camera, boxes in force and erosion element
  cams          run_cams / run_cams_wide with cameras of their own: the context's camera, masks and boxes stay
  first_match   masks at their own size, in host or device memory (device outputs poisoned)
  depth_maps    on the model's camera, with the element in force; behind a call with every mask full, whose counters it must not see;
                with device operands through lpf_depth_maps' device outputs, poisoned, with a capacity some frames overflow
  pairs         match_2d, assign_costs, assign_2d on batch_range_cases' batches, host or device operands
  frame_wide    make_frame_step_wide with NULL corners on the largest frame of the last run (device outputs, poisoned): the boxes in
                force -- refused where they were set for another number of frames than one
  depth_overlays depth_maps, then depth_overlays on ITS lists; refused for host lists with a depth that is not > 0 (depth_min < 0)
  clear_boxes   clear_boxes; inside_masks and box_points are then refused, and the rerun behind it counts no box
  box_views     on the model's camera
  inside_masks  on the lists of the most recent narrow run, host or device operands (device outputs poisoned): the boxes in force
  box_points    on the compact lists of the most recent narrow run, likewise; after a frame step that cleared the boxes both are
                refused ("no boxes in force")
  operators     the stand-alone operators on the state in force: depth_image (camera), prepare_boxes (camera; ``visible`` is
                compared), resize_masks (camera size), erode_masks (element), points_in_boxes
  label         get_label_image: the model's label image.  In order it is read as it stands; under a pipelined mode the op first
                switches the mode off (a switch with work owed) and sets the masks again
  set_element   set_erosion_element: masks already packed keep theirs
  set_pipelined between off, "fused" and "fused-pack" (by a turn, from whatever mode is on)
  sync
With the lab library every op is preceded by set_range_limits, and by set_geometry where the model says nothing is owed (LAB_FORMS,
lab_settings): results must not depend on either.
The camera sizes of a sequence's three narrow cases go large -> small -> larger (scratch sized by W * H is reused at a smaller size and
grown again); at most one set_camera of a sequence goes to 1408 x 376 or 1242 x 375 (at most 8 masks and 2 frames there); the pass,
the reruns and the tail behind it run at that size too, the pass with 33 masks at the most.  All masks of a sequence together stay
under narrow_fuzz_cases.MASK_BYTES.  Mask counts go down and up across 32 between consecutive ops.

LEFT OUT: graph capture (a captured graph's frozen state is a model of its own); lpf_set_stream, lpf_wait_for_stream and
lpf_release_to_stream (only as LpfContext's own calls on GPU operands use them); the reader; RCCL.  NOT BUILT YET, so not covered: the device-output
forms of lpf_run_wide (other than one frame through lpf_run_frame_wide), lpf_run_cams and lpf_run_cams_wide -- LpfContext returns
their results as host arrays."""
import os

import numpy as np

import batch_range_cases as BR
import box_views_ref as BV
import erosion_ref
import box_points_ref as BP
import first_match_ref as FM
import inside_ref as IR
import narrow_fuzz_cases as NG
import overlay_ref as OV
import wide_fuzz_cases as WG
from lidar_object_detection_amd._native import SUMMARY_DTYPE
from oracle import cpu_oracle as orc
from oracle import numpy_path as npp
from test_gpu_depth_maps import _expect

DEFAULT_CASES = 16
DEFAULT_SEED_BASE = 7008                              # a multiple of 16: seed % 16 lays out the values the CPU test counts
MODES = ("off", "fused", "fused-pack")
FAMILIES = ("narrow", "rerun", "rerun-unset", "wide", "cams", "first_match", "depth_maps", "pairs", "box_views", "inside_masks", "box_points",
            "operators", "frame_wide", "depth_overlays", "clear_boxes", "label", "set_element", "set_pipelined", "sync")
PASSES = ("wide", "cams", "first_match", "depth_maps", "pairs", "box_views", "inside_masks", "box_points", "operators", "frame_wide",
          "depth_overlays", "clear_boxes")            # a rerun follows directly
OTHER_FRAMES = "boxes were set for"                   # lpf_run_frame_wide on boxes in force for a batch of several frames
BAD_DEPTH = "finite and > 0"                          # lpf_depth_overlays on host lists, and LpfContext.overlay_rows in front of it
NO_BOXES = "boxes in force"                           # in lpf_inside_masks' "no boxes in force" and in box_points' ValueError
MIN_POINTS = 4
LAB_FORMS = ("auto", "small", "small-narrow", "small-1024", "large", "large-scan")
BIG = [(1408, 376), (1242, 375)]
POISON = 0xA5
REFUSAL = "the masks were set for another scratch set"
PAIR_CALLS = ("match_2d", "assign_costs", "assign_2d")
WIDE_COUNTS = [256, 33, 255, 64, 100, 49, 65, 48]
CAM_SIZES = [(150, 37), (17, 16), (70, 33)]


def default_seeds():
    return [DEFAULT_SEED_BASE + i for i in range(DEFAULT_CASES)]


def seeds():
    """the seeds of this run (LPF_FUZZ_CASES, LPF_FUZZ_SEED_BASE as tests/test_gpu_fuzz.py reads them)"""
    base = int(os.environ.get("LPF_FUZZ_SEED_BASE", str(DEFAULT_SEED_BASE)))
    return [base + i for i in range(int(os.environ.get("LPF_FUZZ_CASES", str(DEFAULT_CASES))))]


# ---- the draws ----------------------------------------------------------------------------------------------------------------------------
def single_frame(cs, f):
    """frame f of a narrow case as a case of its own (make_frame_step takes one frame)"""
    one = dict(cs, F=1, sizes=[cs["sizes"][f]], inside=[cs["inside"][f]], frames=[cs["frames"][f]], on_dmin=[cs["on_dmin"][f]],
               masks=cs["masks"][f:f + 1], member=cs["member"][f:f + 1], cam0=[cs["cam0"][f]])
    one["rects"] = None if cs["rects"] is None else cs["rects"][f:f + 1]
    return one


def _narrow(seed, slot, calib, size, M, element, route):
    """the narrow case of ``slot`` (0, 1, 2): row (3 * seed + slot) % 16 of narrow_fuzz_cases.PLAN at the given camera size, mask
    count and element; a frame step's case has uint8 masks, no erosion and one frame with points"""
    nseed = NG.DEFAULT_SEED_BASE + (3 * seed + slot) % NG.DEFAULT_CASES
    p = NG.plan(nseed)
    over = dict(size=size, M=M, element=element)
    if min(size) < 16:
        over["element"] = 3                                   # (the sequence never has another element in force there: see sequence)
    if size in BIG and p["kind"] != "u8":
        over["kind"] = "u8"
    if route == "step":
        over.update(kind="u8", erode=0)
        over["layout"] = "drawn"                              # frames 0 and 1 are SIZES[s % 10] and SIZES[(s + 4) % 10]: never both empty
        if p["source"] == "label":
            over["source"] = "lent"
    layout = over.get("layout", p["layout"])
    sizes = NG._frame_sizes(nseed, np.random.default_rng(nseed), layout)
    if size in BIG:
        sizes = sizes[:2]
    cs = NG.case(nseed, calib, sizes=sizes, **over)
    assert cs["sizes"] == sizes and (cs["W"], cs["H"]) == size and cs["M"] == M
    if route == "step":
        with_pts = [f for f, n in enumerate(cs["sizes"]) if n]
        assert with_pts, "the layout \"drawn\" has a frame with points among its first two"
        cs = single_frame(cs, next((f for f in with_pts if len(cs["cam0"][f])), with_pts[0]))
    return cs


def _wide_camera(rng, index, calib, sizes, size, M):
    cam = WG._draw_camera(index, rng, calib, sizes, 256, size=size, M=M)
    assert cam["F"] == len(sizes), "the masks of a wide op fit: the draw keeps them small"
    return cam


def _first_match_masks(rng, F, size, index):
    """masks at their OWN size -- smaller than the image, larger, the same -- uint8 or float32 with odd values, and their colours"""
    W, H = size
    mw, mh = [(max(W - 5, 1), max(H - 3, 1)), (W + 7, H + 5), (W, H)][index % 3]
    M = [1, 33, 3, 64, 31, 100][index % 6] if W * H < 100000 else [1, 3][index % 2]
    u8 = WG._draw_masks(rng, F, M, mw, mh)
    if index % 2:
        masks = u8.astype(np.float32)
        masks[:, 0] *= rng.choice(WG.ODD, size=(F, mh, mw))
    else:
        masks = u8 * np.uint8(rng.choice([1, 200, 255]))
    colors = np.ascontiguousarray(rng.integers(0, 256, size=(F, M, 3)).astype(np.float64))
    return masks, colors


class Sequence:
    def __init__(self, seed, ops):
        self.seed, self.ops = seed, ops

    def kinds(self):
        return [op["kind"] for op in self.ops]


def sequence(seed, calib):
    """The seed's ops.  seed % 16 lays out what the CPU test counts: the camera ladder, the routes, the passes between the narrow
    cases (the first two passes are kind seed % 14 of fourteen -- the same call at a large and then at a small camera, with other masks, so that
    the second finds the scratch the first left -- and the third is kind (seed + 4) % 14), the extras; the rest is drawn from default_rng([seed, 1501])."""
    rng = np.random.default_rng([seed, 1501])
    even = seed % 2 == 0
    element_extra = even
    camA = (150, 37) if even else (72, 32)
    camB = (17, 16) if element_extra else [(5, 7), (16, 8), (15, 16)][(seed // 2) % 3]
    camC = BIG[(seed // 2) % 2] if even else (150, 37)
    passes = ["wide", "cams", "cams-wide", "first_match", "depth_maps", "match_2d", "assign_costs", "assign_2d", "box_views", "inside_masks",
              "box_points", "operators", "frame_wide", "depth_overlays"]
    routes = [["device", "host", "device", "device"][seed % 4], "step" if seed % 4 == 1 else "device", ["device", "step"][(seed // 4) % 2]]
    if passes[seed % len(passes)] == "frame_wide":            # behind a batch of several frames it is refused, behind a frame step it runs
        routes[1] = "step"
    if passes[(seed + 4) % len(passes)] == "frame_wide":
        routes[2] = "step"
    Ms = [[1, 3, 8, 9, 16, 17, 32][seed % 7], [32, 1, 17, 9, 0, 16][seed % 6] or (0 if routes[1] != "step" else 8),
          [8, 1, 3][seed % 3] if camC in BIG else [16, 32, 9][seed % 3]]
    ops, element = [], 3
    frames = None

    def narrow(slot, size):
        nonlocal frames
        cs = _narrow(seed, slot, calib, size, Ms[slot], element, routes[slot])
        frames = cs["frames"]
        ops.append(dict(kind="narrow", case=cs, route=routes[slot]))
        return cs

    def a_pass(i, cs):
        kind = passes[(seed + (4 if i == 2 else 0)) % len(passes)]
        sizes, size = cs["sizes"], (cs["W"], cs["H"])
        idx = seed + 5 * i
        if kind == "wide":
            M = WIDE_COUNTS[(seed + 2 * i) % len(WIDE_COUNTS)] if size not in BIG else 33
            ops.append(dict(kind="wide", cam=_wide_camera(rng, idx, calib, sizes, size, M), device=bool(idx % 2)))
        elif kind in ("cams", "cams-wide"):
            n = 1 + idx % 3
            top = 32 if kind == "cams" else 256
            counts = [m for m in WG.MASK_COUNTS if m <= top]
            cams = [_wide_camera(rng, idx + 7 * k, calib, sizes, CAM_SIZES[(idx + k) % 3], counts[(idx + 5 * k) % len(counts)]) for k in range(n)]
            ops.append(dict(kind="cams", wide=kind == "cams-wide", case=dict(seed=seed, frames=cs["frames"], sizes=sizes, cams=cams)))
        elif kind == "first_match":
            masks, colors = _first_match_masks(rng, len(sizes), size, idx)
            ops.append(dict(kind="first_match", masks=masks, colors=colors, device=bool(idx % 2)))
        elif kind == "depth_maps":
            ops.append(dict(kind="depth_maps", cam=_wide_camera(rng, idx, calib, sizes, size, [3, 1, 8][idx % 3]), device=bool(idx % 2),
                            cap=[None, 1][(idx // 2) % 2]))
        elif kind == "box_views":
            I = BR.box_views().inputs
            ops.append(dict(kind="box_views", corners=I["corners"], box_off=I["box_off"], Tcv=I["T_cam_to_velo"], device=bool(idx % 2)))
        elif kind in ("inside_masks", "box_points"):
            ops.append(dict(kind=kind, device=bool(idx % 2)))
        elif kind == "frame_wide":
            f = int(np.argmax(sizes))
            M = WIDE_COUNTS[(seed + 2 * i + 1) % len(WIDE_COUNTS)] if size not in BIG else 33
            ops.append(dict(kind=kind, frame=f, cam=_wide_camera(rng, idx, calib, [sizes[f]], size, M), rects=bool(idx % 2)))
        elif kind == "depth_overlays":
            cam = _wide_camera(rng, idx, calib, sizes, size, [3, 1, 2][idx % 3])
            cam["masks"][:, 0], cam["member"][:, 0] = 1, 1        # car 0 is the whole image: every frame with a valid point has an image
            cam["rects"], cam["rects_mode"] = None, "none"       # (the drawn rectangles were those of the drawn masks)
            ops.append(dict(kind=kind, cam=cam, device=bool(idx % 2),
                            seg=rng.integers(0, 256, size=(len(sizes), size[1], size[0], 3), dtype=np.uint8)))
        elif kind == "operators":
            w, h = max(size[0] // 2, 3), max(size[1] // 2 + 1, 2)
            ops.append(dict(kind=kind, device=bool(idx % 2), small=rng.integers(0, 256, size=(2, h, w), dtype=np.uint8),
                            planes=WG._draw_masks(rng, 1, 3, 37, 21)[0] * np.uint8(255), iters=1 + idx % 2))
        else:
            ops.append(dict(kind="pairs", call=kind, place=["hh", "dd"][idx % 2]))
        ops.append(dict(kind="rerun"))

    csA = narrow(0, camA)
    ops.append(dict(kind="rerun"))
    a_pass(0, csA)
    if seed % 4 == 1:
        ops.append(dict(kind="sync"))
    if element_extra:                                         # an element change between a pack and its rerun
        element = 5
        ops += [dict(kind="set_element", k=5), dict(kind="rerun")]
    if seed % 4 == 3:
        ops.append(dict(kind="rerun-unset"))
    csB = narrow(1, camB)
    a_pass(1, csB)
    if seed % 4 != 2:
        ops.append(dict(kind="set_pipelined", turn=1 + (seed // 4) % 2))       # directly behind a run: its tail is owed
    csC = narrow(2, camC)
    a_pass(2, csC)
    if seed % 4 == 2:
        ops.append(dict(kind="label"))
    if seed % 4 == 3:
        ops += [dict(kind="clear_boxes"), dict(kind="rerun")]
    assert 10 <= len(ops) <= 14, (seed, len(ops))
    return Sequence(seed, ops)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
def _camera_of(cs):
    return dict(T=cs["T"], K=cs["K"], W=cs["W"], H=cs["H"], dmin=cs["dmin"], dmax=cs["dmax"])


def wide_reference(cam, frames, camera, boxes, element):
    """run_wide's reference for the state in force: the op's masks (cam) eroded with the context's ``element``, the model's camera
    and the boxes in force -- dropped boxes keep their column, as narrow_fuzz_cases.reference maps them"""
    state = dict(cam, **camera)
    out = []
    for f, pts in enumerate(frames):
        mem = (np.asarray(cam["member"][f]) != 0).astype(np.uint8)
        if cam["erode"] and len(mem):
            mem = erosion_ref.erode(mem, element, cam["erode"])
        keep, velo = boxes["keep"][f], boxes["velo"][f]
        r = WG.oracle_result(dict(state, boxes=[velo[keep]], oriented=boxes["oriented"]), pts, 0, member=mem)
        pos = np.flatnonzero(keep)
        full = np.zeros((len(mem), len(keep)), np.int64)
        full[:, keep] = r["count_mb"]
        r["count_mb"] = full
        r["best_box"] = np.where(r["best_box"] >= 0, pos[np.maximum(r["best_box"], 0)] if len(pos) else -1, -1).astype(np.int32)
        out.append(r)
    return out


def first_match_reference(refs, frames, masks, colors):
    """lpf_first_match's outputs in the layout the call writes them, from first_match_ref on the narrow reference's pixels (the
    model's camera and depth window); ``count``: per output the entries of each frame the call writes"""
    F, M = masks.shape[:2]
    off = np.concatenate([[0], np.cumsum([len(p) for p in frames])]).astype(np.int64)
    per = []
    for f, p in enumerate(frames):
        valid = np.zeros(len(p), bool)
        valid[refs[f]["valid_idx"]] = True
        per.append(FM.first_match(refs[f]["u"], refs[f]["v"], valid, list(masks[f])))
    return dict(off=off, per=per, M=M)


def _corners_in_force(boxes, f):
    """frame f's boxes as the tables hold them: a box the visibility filter dropped keeps its position and holds nothing"""
    velo = np.array(boxes["velo"][f], np.float64).reshape(-1, 8, 3)
    velo[~boxes["keep"][f]] = 1e9
    return velo


def inside_reference(cs, refs, boxes):
    """lpf_inside_masks on the run's own lists: inputs (the reference's lists in the layout the run writes them) and the outputs in
    the call's layout from inside_ref.frame_split on the boxes in force; cap: the largest frame's need and three, so every frame fits"""
    F, M = cs["F"], cs["M"]
    cap = max(r["need"] for r in refs) + 3                  # (room behind every frame's lists: the poison has to stay there)
    inp = dict(inst_idx=np.zeros((F, cap), np.int64), inst_off=np.zeros((F, M + 1), np.int64), best_box=np.full((F, M), -1, np.int32),
               best_cnt=np.zeros((F, M), np.int64))
    ref = dict(inside=[], part_idx=[], part_xyz=[], n_inside=np.zeros((F, M), np.int64), matched=np.zeros((F, M), np.int32))
    for f, r in enumerate(refs):
        with np.errstate(invalid="ignore", divide="ignore"):  # (a dropped box has no extent)
            s = IR.frame_split(cs["frames"][f], r["inst_lists"], _corners_in_force(boxes, f), MIN_POINTS, boxes["oriented"])
        assert np.array_equal(s["count_mb"], r["count_mb"]), "inside_ref counts what the oracle counts"
        n = r["need"]
        inp["inst_idx"][f, :n] = np.concatenate([np.zeros(0, np.int64)] + list(r["inst_lists"]))
        inp["inst_off"][f], inp["best_box"][f], inp["best_cnt"][f] = s["off"], r["best_box"], r["best_cnt"]
        ref["n_inside"][f], ref["matched"][f] = s["n_inside"], s["matched"]
        for k in ("inside", "part_idx", "part_xyz"):
            ref[k].append(s[k])
    return dict(inputs=inp, ref=ref, cap=cap)


def box_points_reference(cs, refs, boxes):
    """lpf_box_points on the run's own compact lists: inputs and the outputs from box_points_ref on the boxes in force"""
    off = np.concatenate([[0], np.cumsum(cs["sizes"])]).astype(np.int64)
    Ntot, F = int(off[-1]), cs["F"]
    inp = dict(valid_idx=np.zeros(Ntot, np.int64), n_valid=np.zeros(F, np.int64), label_valid=np.zeros(Ntot, np.uint32))
    ref = dict(box_points=[], box_labelled=[], first_box=[], frame_counts=np.zeros((F, 4), np.int64))
    for f, r in enumerate(refs):
        a, nv = int(off[f]), r["n_valid"]
        inp["valid_idx"][a:a + nv], inp["label_valid"][a:a + nv], inp["n_valid"][f] = r["valid_idx"], r["label_valid"], nv
        s = BP.frame_box_points(cs["frames"][f], r["valid_idx"], boxes["velo"][f], r["label_valid"] != 0, boxes["oriented"], enabled=boxes["keep"][f])
        ref["frame_counts"][f] = s["frame_counts"]
        for k in ("box_points", "box_labelled", "first_box"):
            ref[k].append(s[k])
    ref["box_points"] = np.concatenate(ref["box_points"]).astype(np.int32)
    ref["box_labelled"] = np.concatenate(ref["box_labelled"]).astype(np.int32)
    return dict(inputs=inp, ref=ref, off=off)


def check_inside(got, e, what, poison):
    """lpf_inside_masks' outputs: every row up to the frame's need, bit for bit; beyond it the poison (device outputs)"""
    ref = e["ref"]
    for k in ("n_inside", "matched"):
        assert np.array_equal(np.asarray(got[k]).reshape(ref[k].shape), ref[k]), (what, k)
    for f in range(len(ref["inside"])):
        n = len(ref["inside"][f])
        for k in ("inside", "part_idx", "part_xyz"):
            g = np.asarray(got[k])[f]
            assert g[:n].tobytes() == np.ascontiguousarray(ref[k][f], g.dtype).tobytes(), (what, f, k)
            if poison:
                assert _intact(g[n:]), (what, f, k, "written beyond the frame's lists")


def check_box_points(got, e, what, poison):
    ref, off = e["ref"], e["off"]
    for k in ("box_points", "box_labelled", "frame_counts"):
        assert np.array_equal(np.asarray(got[k]).reshape(ref[k].shape), ref[k]), (what, k)
    first = np.asarray(got["first_box"])
    for f, want in enumerate(ref["first_box"]):
        a, b = int(off[f]), int(off[f + 1])
        assert np.array_equal(first[a:a + len(want)], want), (what, f, "first_box")
        if poison:
            assert _intact(first[a + len(want):b]), (what, f, "first_box", "written beyond n_valid")


def forge_inside(e):
    """the outputs a correct lpf_inside_masks leaves in poisoned device arrays (tests of the checker)"""
    F, M = e["ref"]["n_inside"].shape
    h = dict(inside=poisoned((F, e["cap"]), np.uint8), part_idx=poisoned((F, e["cap"]), np.int64), part_xyz=poisoned((F, e["cap"], 3), np.float32),
             n_inside=e["ref"]["n_inside"].copy(), matched=e["ref"]["matched"].copy())
    for f in range(F):
        for k in ("inside", "part_idx", "part_xyz"):
            h[k][f, :len(e["ref"][k][f])] = e["ref"][k][f]
    return h


def forge_box_points(e):
    ref = e["ref"]
    h = dict(box_points=ref["box_points"].copy(), box_labelled=ref["box_labelled"].copy(), frame_counts=ref["frame_counts"].copy(),
             first_box=poisoned((int(e["off"][-1]),), np.int32))
    for f, want in enumerate(ref["first_box"]):
        h["first_box"][int(e["off"][f]):int(e["off"][f]) + len(want)] = want
    return h


def maps_shapes(F, M, cap):
    """lpf_depth_maps' device outputs; the three lists have a GUARD ROW behind the last frame's, which must keep its poison: what an
    overflowing frame would write at or beyond cap lands in the next row"""
    return dict(pix=((F + 1, cap), np.int64), depth=((F + 1, cap), np.float64), point_idx=((F + 1, cap), np.int64), car_off=((F, M + 1), np.int64),
                need=((F,), np.int64), overflow=((F,), np.int32))


def check_maps_device(h, want, cap, what):
    """lpf_depth_maps' device outputs: car_off, need and overflow of every frame; the lists of a frame that fits, bit for bit, and the
    poison behind them up to cap (lpf.h: "entries at or beyond cap are not written", and nothing is beyond a frame's need)"""
    for f, fr in enumerate(want):
        off = np.concatenate([[0], np.cumsum([len(car[0]) for car in fr])]).astype(np.int64)
        need = int(off[-1])
        assert np.array_equal(h["car_off"][f], off) and int(h["need"][f]) == need, (what, f, "car_off, need")
        assert int(h["overflow"][f]) == int(need > cap), (what, f, "overflow")
        nxt = next((g for g in range(f + 1, len(want)) if sum(len(car[0]) for car in want[g]) <= cap), len(want))
        if need > cap:                                        # its row is not compared; the next row that is checked whole is row nxt:
            for k in ("pix", "depth", "point_idx"):           # a fitting frame's (below) or the guard row
                assert nxt < len(want) or _intact(h[k][len(want)]), (what, f, k, "written at or beyond cap")
            continue
        for k, j, dt in (("pix", 0, np.int64), ("depth", 1, np.float64), ("point_idx", 2, np.int64)):
            flat = np.concatenate([np.zeros(0, dt)] + [np.asarray(car[j], dt) for car in fr])
            assert h[k][f, :need].tobytes() == flat.tobytes(), (what, f, k)
            assert _intact(h[k][f, need:]), (what, f, k, "written beyond need")
    for k in ("pix", "depth", "point_idx"):
        assert _intact(h[k][len(want)]), (what, k, "the guard row behind the last frame was written")


def forge_maps_device(want, cap):
    F, M = len(want), len(want[0])
    h = {k: poisoned(*sd) for k, sd in maps_shapes(F, M, cap).items()}
    for f, fr in enumerate(want):
        off = np.concatenate([[0], np.cumsum([len(car[0]) for car in fr])]).astype(np.int64)
        h["car_off"][f], h["need"][f], h["overflow"][f] = off, off[-1], int(off[-1] > cap)
        if off[-1] <= cap:
            for k, j in (("pix", 0), ("depth", 1), ("point_idx", 2)):
                h[k][f, :off[-1]] = np.concatenate([np.zeros(0)] + [np.asarray(car[j]) for car in fr])
    return h


FRAME_WIDE_LISTS = ("valid_idx", "uv_valid", "label_valid_words")


def frame_wide_result(h, M, B):
    """lpf_run_frame_wide's device outputs (NumPy copies) as one frame's dict in run_wide's shape"""
    nv = int(h["n_valid"][0])
    io = h["inst_off"]
    return dict(u=h["uv"][:, 0], v=h["uv"][:, 1], depth=h["depth"], uf=h["u_f"], vf=h["v_f"], label_words=h["label_words"].view(np.uint32),
                valid_idx=h["valid_idx"][:nv], count_mb=h["count_mb"].reshape(M, B), best_box=h["best_box"], best_cnt=h["best_cnt"],
                inst_count=h["inst_count"], n_valid=nv, n_labelled=int(h["n_labelled"][0]),
                inst_lists=[h["inst_idx"][io[m]:io[m + 1]] for m in range(M)], label_valid_words=h["label_valid_words"][:nv].view(np.uint32),
                u_valid=h["uv_valid"][:nv, 0], v_valid=h["uv_valid"][:nv, 1])


def check_frame_wide(h, ref, M, B, what):
    """a wide frame step's device outputs against the reference, and the poison behind n_valid and behind the instance lists"""
    assert int(h["inst_overflow"][0]) == 0, (what, "inst_overflow")
    try:
        WG.compare(frame_wide_result(h, M, B), ref, what)
    except AssertionError as e:
        raise AssertionError((what,) + tuple(e.args)) from None
    assert np.array_equal(h["inst_off"], np.concatenate([[0], np.cumsum(ref["inst_count"])])), (what, "inst_off")
    for k in FRAME_WIDE_LISTS:
        assert _intact(h[k][ref["n_valid"]:]), (what, k, "written beyond n_valid")
    assert _intact(h["inst_idx"][int(ref["inst_count"].sum()):]), (what, "inst_idx", "written beyond the lists")


def forge_frame_wide(ref, n, M, B, cap):
    LW = (M + 31) // 32
    nv, need = ref["n_valid"], int(ref["inst_count"].sum())
    h = dict(uv=np.stack([ref["u"], ref["v"]], axis=1).astype(np.int32), depth=ref["depth"].copy(), u_f=ref["uf"].copy(), v_f=ref["vf"].copy(),
             label_words=ref["label_words"].view(np.int32).reshape(n, LW).copy(), valid_idx=poisoned((n,), np.int64), uv_valid=poisoned((n, 2), np.int32),
             label_valid_words=poisoned((n, LW), np.int32), inst_idx=poisoned((cap,), np.int64), count_mb=ref["count_mb"].astype(np.int32).reshape(-1),
             n_valid=np.array([nv], np.int64), n_labelled=np.array([ref["n_labelled"]], np.int64), inst_count=ref["inst_count"].astype(np.int64),
             inst_off=np.concatenate([[0], np.cumsum(ref["inst_count"])]).astype(np.int64), best_cnt=ref["best_cnt"].astype(np.int64),
             best_box=ref["best_box"].astype(np.int32), inst_overflow=np.zeros(1, np.int32))
    h["valid_idx"][:nv] = ref["valid_idx"]
    h["uv_valid"][:nv, 0], h["uv_valid"][:nv, 1] = ref["u_valid"], ref["v_valid"]
    h["label_valid_words"][:nv] = ref["label_valid_words"].view(np.int32).reshape(nv, LW)
    h["inst_idx"][:need] = np.concatenate([np.zeros(0, np.int64)] + list(ref["inst_lists"]))
    return h


def check_cams(op, res, refs, what):
    """every camera of a run_cams / run_cams_wide pass against its reference"""
    assert len(res) == len(refs), (what, "cameras")
    for k, (got, want) in enumerate(zip(res, refs)):
        assert len(got) == len(want), (what, k, "frames")
        for f in range(len(want)):
            try:
                (WG.compare if op["wide"] else WG.compare_narrow)(got[f], want[f], ("camera %d" % k, f))
            except AssertionError as e:
                raise AssertionError((what,) + tuple(e.args)) from None


def check_label(got, want, what):
    assert np.asarray(got).shape == want.shape and np.array_equal(got, want), (what, "label image")


def check_operators(got, ref, what):
    for k, want in ref.items():
        g = np.asarray(got[k])
        assert g.shape == want.shape and g.astype(want.dtype).tobytes() == want.tobytes(), (what, k)


def lab_settings(seed, i, idle):
    """what a lab run sets before op i: (geometry or None where work is owed, staging budget in bytes, max_items)"""
    rng = np.random.default_rng([seed, 77, i])
    form = LAB_FORMS[int(rng.integers(0, len(LAB_FORMS)))] if idle else None
    return form, int(rng.choice([0, 1, 4096, 1 << 20])), int(rng.choice([0, 1, 2, 3]))


class Model:
    """The documented state of one context.  apply(op) returns what the op must give for the state in force -- dict(kind, setup: the
    set-up calls the op makes, refuse: the message of a documented refusal or None, and the references) -- and moves the state on."""

    def __init__(self, mode="off"):
        assert mode in MODES
        self.mode, self.element = mode, 3
        self.camera = self.case = self.refs = self.boxes = None
        self.masks_live = False                               # the masks in force serve the next run as they stand
        self.owed = False                                     # a pipelined run's tail has not been launched
        self.step = False                                     # the last narrow run was a frame step

    def _narrow_refs(self, cs):
        return NG.reference(cs)

    def apply(self, op):
        """the op's expectation, with ``idle``: nothing was owed when the op began (a lab run may change the launch geometry there)"""
        idle = not self.owed
        e = self._apply(op)
        e["idle"] = idle
        return e

    def _apply(self, op):
        kind = op["kind"]
        if kind == "narrow":
            # lpf.h, lpf_set_masks_*: "erode_iters: iterations of cv2.erode with the context's erosion element"
            cs = dict(op["case"], element=self.element)
            route = op["route"] if (op["route"] != "host" or self.mode == "off") else "device"
            source = "lent" if (cs["source"] == "label" and self.mode != "off") else cs["source"]
            self.case, self.refs, self.camera = cs, self._narrow_refs(cs), _camera_of(cs)
            self.boxes = dict(velo=[r["corners_velo"] for r in self.refs], keep=[r["visible"] for r in self.refs], oriented=cs["oriented"],
                              none=route == "step" and len(cs["cam0"][0]) == 0)      # (a frame step without boxes clears them)
            self.masks_live, self.owed, self.step = True, self.mode != "off", route == "step"
            return dict(kind=kind, route=route, source=source, setup=("camera", "masks", "boxes"), refuse=None, case=cs, refs=self.refs)
        if kind in ("rerun", "rerun-unset"):
            cs = self.case
            if kind == "rerun-unset" and self.mode != "off" and cs["M"] > 0:
                # lpf.h, lpf_set_pipelined: "the label images rotate with the scratch sets (call lpf_set_masks_* before every lpf_run*
                # while a pipelined mode is on)"
                return dict(kind=kind, route="device", setup=(), refuse=REFUSAL, case=cs, refs=self.refs)
            again = kind == "rerun" and (self.mode != "off" or not self.masks_live)
            if kind == "rerun-unset" and not self.masks_live:
                again = True                                  # (in order after a mode switch: nothing is in force, the masks come again)
            if again and cs["element"] != self.element:
                # lpf.h, lpf_set_erosion_element: "Masks already packed keep the element they were packed with" -- masks set again
                # take the element now in force
                cs = dict(cs, element=self.element)
                self.case, self.refs = cs, self._narrow_refs(cs)
            source = "lent" if (cs["source"] == "label" and self.mode != "off") else cs["source"]
            route = "step-null" if (self.step and not again and cs["M"] > 0) else "device"
            self.masks_live, self.owed = True, self.mode != "off"
            # lpf.h, lpf_set_pipelined: "boxes that are not set again stay in force"
            return dict(kind=kind, route=route, source=source, setup=("masks",) if again else (), refuse=None, case=cs, refs=self.refs)
        if kind == "set_element":
            self.element = op["k"]
            return dict(kind=kind, setup=(), refuse=None)
        if kind == "set_pipelined":
            owed = self.owed
            self.mode = MODES[(MODES.index(self.mode) + op["turn"]) % len(MODES)]
            self.masks_live, self.owed = False, False         # lpf_api.hip's refusal: "call lpf_set_masks_* ... (and after switching modes)"
            return dict(kind=kind, mode=self.mode, owed=owed, setup=(), refuse=None)
        if kind == "sync":
            self.owed = False
            return dict(kind=kind, setup=(), refuse=None)
        if kind == "clear_boxes":
            # lpf.h, lpf_inside_masks / lpf_box_points: "LPF_ERR_STATE: no boxes in force"; the run behind it counts no box
            cs = dict(self.case, cam0=[np.zeros((0, 8, 3)) for _ in self.case["cam0"]])
            self.case, self.refs = cs, self._narrow_refs(cs)
            self.boxes = dict(velo=[r["corners_velo"] for r in self.refs], keep=[r["visible"] for r in self.refs], oriented=cs["oriented"], none=True)
            return dict(kind=kind, setup=(), refuse=NO_BOXES, frames=cs["frames"])
        if kind == "label":
            setup = ()
            if self.mode != "off":
                self.mode, self.masks_live, self.owed = "off", False, False
                setup += ("pipelined-off",)
            cs = self.case
            if not self.masks_live:
                setup += ("masks",)
                if cs["element"] != self.element:
                    cs = dict(cs, element=self.element)
                    self.case, self.refs = cs, self._narrow_refs(cs)
            self.masks_live = True
            want = np.stack([r["label_img"] for r in self.refs])
            return dict(kind=kind, setup=setup, refuse=None, case=cs, source=cs["source"], refs=self.refs, label=want)
        # the passes: lpf.h, "with a software-pipelined mode on it first launches what the pipeline owes", and every one of them leaves
        # "the masks, boxes and rectangles of the narrow calls as they were"
        self.owed = False
        frames = self.case["frames"]
        if kind == "wide":
            # lpf.h, lpf_run_wide: "the boxes are the ones in force (lpf_set_boxes*), the camera and depth window the ones of lpf_set_camera"
            refs = wide_reference(op["cam"], frames, self.camera, self.boxes, self.element)
            return dict(kind=kind, setup=(), refuse=None, refs=refs, frames=frames)
        if kind == "cams":
            # lpf.h, lpf_run_cams: "The context's camera, masks, rectangles and boxes in force are left as they were"; the cameras'
            # erosion is the context's element (lpf_set_erosion_element: "the erode_iters of a lpf_wide_input")
            refs = []
            for cam in op["case"]["cams"]:
                own = dict(velo=cam["boxes"], keep=[np.ones(len(b), bool) for b in cam["boxes"]], oriented=cam["oriented"])
                refs.append(wide_reference(cam, frames, _camera_of(cam), own, self.element))
            return dict(kind=kind, setup=(), refuse=None, refs=refs, frames=frames)
        if kind == "first_match":
            # lpf.h, lpf_first_match: "Entries of a frame's span at or beyond its count are NOT WRITTEN"
            return dict(kind=kind, setup=(), refuse=None, ref=first_match_reference(self.refs, frames, op["masks"], op["colors"]), frames=frames)
        if kind == "depth_maps":
            # the call goes twice: first with every mask full (the "primer": every (mask, tile) that has a winning point counts), then with
            # the op's masks -- counters the primer left behind must not show where the op's masks have no member
            cam, c = op["cam"], self.camera
            want, primer = [], []
            for f, pts in enumerate(frames):
                D, win = orc.depth_image(pts, c["T"], c["K"], c["W"], c["H"], c["dmin"], c["dmax"])
                mem = (np.asarray(cam["member"][f]) != 0).astype(np.uint8)
                if cam["erode"]:
                    mem = erosion_ref.erode(mem, self.element, cam["erode"])
                want.append(_expect(D, win, mem.astype(bool)))
                primer.append(_expect(D, win, np.ones(mem.shape, bool)))
            needs = [sum(len(car[0]) for car in fr) for fr in want]
            cap = (tight_cap(needs) if op["cap"] == 1 else None) or max(needs) + 3
            return dict(kind=kind, setup=(), refuse=None, maps=want, primer=primer, frames=frames, dev_cap=cap)
        if kind == "pairs":
            return dict(kind=kind, setup=(), refuse=None, ref=BR.case(op["call"]).ref)
        if kind == "frame_wide":
            # lpf.h, lpf_run_frame_wide: "a NULL corners_cam0 leaves the boxes in force as they are; the masks, rectangles and label
            # state of the narrow calls are left as they were"; boxes in force for a batch of several frames are for another run
            f = op["frame"]
            if not self.boxes["none"] and len(self.boxes["velo"]) != 1:
                return dict(kind=kind, setup=(), refuse=OTHER_FRAMES, pts=frames[f])
            cam = dict(op["cam"], erode=0)
            refs = wide_reference(cam, [frames[f]], self.camera, self.boxes, self.element)
            return dict(kind=kind, setup=(), refuse=None, pts=frames[f], ref=refs[0], cap=int(refs[0]["inst_count"].sum()) + 3,
                        B=len(self.boxes["velo"][0]))
        if kind == "depth_overlays":
            cam, c = op["cam"], self.camera
            want = []
            for f, pts in enumerate(frames):
                D, win = orc.depth_image(pts, c["T"], c["K"], c["W"], c["H"], c["dmin"], c["dmax"])
                mem = (np.asarray(cam["member"][f]) != 0).astype(np.uint8)
                if cam["erode"]:
                    mem = erosion_ref.erode(mem, self.element, cam["erode"])
                want.append(_expect(D, win, mem.astype(bool)))
            if any((car[1] <= 0).any() for fr in want for car in fr):
                # lpf.h, lpf_depth_overlays: "Lists in host memory are checked (... depths finite and > 0: LPF_ERR_ARG otherwise)"
                return dict(kind=kind, setup=(), refuse=BAD_DEPTH, maps=want, frames=frames)
            lut = OV.jet_lut()
            M = cam["M"]
            images = np.zeros((len(frames), M, c["H"], c["W"], 3), np.uint8)
            mx = np.zeros((len(frames), M))
            for f, fr in enumerate(want):
                for m, car in enumerate(fr):
                    images[f, m], mx[f, m] = OV.overlay(op["seg"][f], car[0], car[1], lut)
            return dict(kind=kind, setup=(), refuse=None, maps=want, frames=frames, ref=dict(images=images, max_depth=mx))
        if kind in ("inside_masks", "box_points"):
            # lpf.h, lpf_inside_masks / lpf_box_points: "the boxes and the `oriented` flag are the ones in force (lpf_set_boxes*)";
            # "LPF_ERR_STATE: no boxes in force"
            if self.boxes["none"]:
                return dict(kind=kind, setup=(), refuse=NO_BOXES, frames=frames)
            make = inside_reference if kind == "inside_masks" else box_points_reference
            return dict(kind=kind, setup=(), refuse=None, frames=frames, **make(self.case, self.refs, self.boxes))
        if kind == "operators":
            c, b = self.camera, self.boxes
            f = int(np.argmax(self.case["sizes"]))
            D, win = orc.depth_image(frames[f], c["T"], c["K"], c["W"], c["H"], c["dmin"], c["dmax"])
            visible = npp.prepare_boxes(self.case["cam0"][0], c["K"], c["W"], c["H"], self.case["TrVeloToCam"])[0]
            resized = np.stack([npp.cv2_resize_linear_u8(m, c["W"], c["H"]) for m in op["small"]])
            # lpf.h, lpf_set_erosion_element: "From then on every erosion of the context uses it: ... and lpf_erode_masks_u8"
            eroded = erosion_ref.erode(op["planes"], self.element, op["iters"])
            pts = frames[f][:200]
            inside = np.stack([orc.points_in_box(pts, box, b["oriented"]) for box in b["velo"][0]]) if len(b["velo"][0]) and len(pts) \
                else np.zeros((len(b["velo"][0]), len(pts)), bool)
            return dict(kind=kind, setup=(), refuse=None, frame=f, frames=frames, cam0=self.case["cam0"][0], Tcv=self.case["Tcv"], velo=b["velo"][0],
                        oriented=b["oriented"], ref=dict(D=D, win=win.astype(np.int32), visible=np.asarray(visible, bool),
                                                                          resized=resized, eroded=eroded, inside=inside))
        if kind == "box_views":
            c = self.camera
            r = BV.views(op["corners"], op["box_off"], c["K"], c["W"], c["H"], op["Tcv"])
            return dict(kind=kind, setup=(), refuse=None, ref={k: np.ascontiguousarray(r[k]) for k in BV.WANT})
        raise KeyError(kind)


def tight_cap(needs):
    """a capacity below the largest frame's need at which the frames that need less fit (None where no frame needs two entries)"""
    big = max(needs)
    return None if big < 2 else max(max((n for n in needs if n < big), default=0), big // 2, 1)


def expectations(seq, mode):
    """what every op of the sequence must give on a context that starts in ``mode``"""
    model = Model(mode)
    return [model.apply(op) for op in seq.ops]


# ---- device outputs: buffers, poison, the checker -------------------------------------------------------------------------------------------
def capacity(cs, refs):
    """(inst_cap, tight) as tests/test_gpu_fuzz_narrow.py chooses it: odd seeds run with less than the largest frame needs"""
    cap = NG.tight_inst_cap(refs) if cs["tight_cap"] else None
    return (cap, True) if cap is not None else (max(max(r["need"] for r in refs), 1), False)


def narrow_shapes(cs, fields, cap):
    """name -> (shape, dtype) of the device outputs ``fields`` (and the summary) of a run of the case"""
    n, F, M = max(int(sum(cs["sizes"])), 1), cs["F"], cs["M"]
    Btot = sum(len(c) for c in cs["cam0"])
    shapes = dict(uv=((n, 2), np.int32), label_bits=((n,), np.int32), depth=((n,), np.float64), u_f=((n,), np.float64), v_f=((n,), np.float64),
                  valid_idx=((n,), np.int64), inst_idx=((F, cap), np.int64), count_mb=((max(M * Btot, 1),), np.int32),
                  uv_valid=((n, 2), np.int32), label_valid=((n,), np.int32))
    out = {k: shapes[k] for k in fields}
    out["summary"] = ((F * SUMMARY_DTYPE.itemsize,), np.uint8)
    return out


def poisoned(shape, dtype):
    a = np.empty(shape, dtype)
    a.view(np.uint8).reshape(-1)[:] = POISON
    return a


def _intact(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == POISON).all())


def read_narrow(cs, h, what):
    """the device outputs of a run (NumPy copies, name -> array) as one dict per frame, keys as run_batch names them"""
    M, sizes = cs["M"], cs["sizes"]
    sm = np.frombuffer(h["summary"].tobytes(), SUMMARY_DTYPE)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    boff = np.concatenate([[0], np.cumsum([len(c) for c in cs["cam0"]])]).astype(np.int64)
    got = []
    for f in range(len(sizes)):
        a, b, s = int(off[f]), int(off[f + 1]), sm[f]
        nv = int(s["n_valid"])
        assert 0 <= nv <= b - a, (what, f, "n_valid", nv)
        r = dict(n_valid=nv, n_labelled=int(s["n_labelled"]), inst_count=s["inst_count"][:M], best_box=s["best_box"][:M], best_cnt=s["best_cnt"][:M],
                 inst_overflow=int(s["inst_overflow"]))
        if "uv" in h:
            r.update(u=h["uv"][a:b, 0], v=h["uv"][a:b, 1])
        if "label_bits" in h:
            r["label_bits"] = h["label_bits"][a:b].view(np.uint32)
        for k, name in (("depth", "depth"), ("u_f", "uf"), ("v_f", "vf")):
            if k in h:
                r[name] = h[k][a:b]
        if "valid_idx" in h:
            r["valid_idx"] = h["valid_idx"][a:a + nv]
        if "uv_valid" in h:
            r.update(u_valid=h["uv_valid"][a:a + nv, 0], v_valid=h["uv_valid"][a:a + nv, 1])
        if "label_valid" in h:
            r["label_valid"] = h["label_valid"][a:a + nv].view(np.uint32)
        if "inst_idx" in h:
            io = s["inst_off"]
            r["inst_lists"] = [h["inst_idx"][f, int(io[m]):int(io[m + 1])] for m in range(M)]
        if "count_mb" in h:
            r["count_mb"] = h["count_mb"][M * int(boff[f]):M * int(boff[f + 1])].reshape(M, int(boff[f + 1] - boff[f]))
        got.append(r)
    return got


def check_narrow(cs, h, refs, cap, what, visible=None):
    """The device outputs ``h`` of a narrow run against the reference, bit for bit (narrow_fuzz_cases.check), and the poison where
    nothing is written: the compact lists beyond n_valid, a fitting frame's instance lists beyond its need, count_mb beyond M * Btot."""
    got = read_narrow(cs, h, what)
    if visible is not None:
        for f, r in enumerate(got):
            r["visible"] = visible[f]
    try:
        NG.check(cs, got, refs, route=str(what), inst_cap=cap if "inst_idx" in h else None)
    except AssertionError as e:
        raise AssertionError((what,) + tuple(e.args)) from None
    off = np.concatenate([[0], np.cumsum(cs["sizes"])]).astype(np.int64)
    for f, ref in enumerate(refs):
        a, b, nv = int(off[f]), int(off[f + 1]), ref["n_valid"]
        for k in ("valid_idx", "uv_valid", "label_valid"):
            if k in h:
                assert _intact(h[k][a + nv:b]), (what, f, k, "written beyond n_valid")
        if "inst_idx" in h and ref["need"] <= cap:
            assert _intact(h["inst_idx"][f, ref["need"]:]), (what, f, "inst_idx", "written beyond the lists")
    Btot = sum(len(c) for c in cs["cam0"])
    if "count_mb" in h:
        assert _intact(h["count_mb"][cs["M"] * Btot:]), (what, "count_mb", "written beyond M * Btot")
    if not sum(cs["sizes"]):
        for k in ("uv", "label_bits", "depth", "u_f", "v_f", "valid_idx", "uv_valid", "label_valid"):
            if k in h:
                assert _intact(h[k]), (what, k, "written without points")


def forge_narrow(cs, refs, fields, cap):
    """the device outputs a correct run leaves in poisoned buffers: what check_narrow has to pass (tests of the checker)"""
    h = {k: poisoned(*sd) for k, sd in narrow_shapes(cs, fields, cap).items()}
    sm = np.zeros(cs["F"], SUMMARY_DTYPE)
    off = np.concatenate([[0], np.cumsum(cs["sizes"])]).astype(np.int64)
    boff = np.concatenate([[0], np.cumsum([len(c) for c in cs["cam0"]])]).astype(np.int64)
    M = cs["M"]
    for f, ref in enumerate(refs):
        a, b, nv = int(off[f]), int(off[f + 1]), ref["n_valid"]
        over = ref["need"] > cap
        s = sm[f]
        s["n_valid"], s["n_labelled"], s["inst_overflow"] = nv, ref["n_labelled"], int(over and "inst_idx" in h)
        s["inst_count"][:M], s["best_box"][:M], s["best_cnt"][:M] = ref["inst_count"], ref["best_box"], ref["best_cnt"]
        s["inst_off"][:M + 1] = np.concatenate([[0], np.cumsum(ref["inst_count"])])
        if "uv" in h:
            h["uv"][a:b, 0], h["uv"][a:b, 1] = ref["u"], ref["v"]
        if "label_bits" in h:
            h["label_bits"][a:b] = ref["label_bits"].view(np.int32)
        for k, name in (("depth", "depth"), ("u_f", "uf"), ("v_f", "vf")):
            if k in h:
                h[k][a:b] = ref[name]
        if "valid_idx" in h:
            h["valid_idx"][a:a + nv] = ref["valid_idx"]
        if "uv_valid" in h:
            h["uv_valid"][a:a + nv, 0], h["uv_valid"][a:a + nv, 1] = ref["u_valid"], ref["v_valid"]
        if "label_valid" in h:
            h["label_valid"][a:a + nv] = ref["label_valid"].view(np.int32)
        if "inst_idx" in h and not over and M:
            h["inst_idx"][f, :ref["need"]] = np.concatenate([np.zeros(0, np.int64)] + list(ref["inst_lists"]))
        if "count_mb" in h:
            h["count_mb"][M * int(boff[f]):M * int(boff[f + 1])] = ref["count_mb"].reshape(-1)
    h["summary"] = np.frombuffer(sm.tobytes(), np.uint8).copy()
    return h


FM_PER_POINT = {"car_idx": "car", "car_mask": "car", "car_xyz": "car", "car_rgb": "car", "bg_idx": "bg", "bg_xyz": "bg"}
FM_PER_FRAME = {"n_valid": ("F",), "n_car": ("F",), "n_bg": ("F",), "mask_count": ("F", "M")}       # int64, written for every frame
FM_SHAPES = {"first_mask": ((), np.int32), "car_idx": ((), np.int64), "car_mask": ((), np.int32), "car_xyz": ((3,), np.float32),
             "car_rgb": ((3,), np.float64), "bg_idx": ((), np.int64), "bg_xyz": ((3,), np.float32)}


def first_match_rows(ref, frames, colors, f):
    """frame f's rows of every per-point output of lpf_first_match"""
    r, p = ref["per"][f], frames[f]
    return dict(first_mask=r["first_mask"], car_idx=r["car_idx"], car_mask=r["car_mask"], car_xyz=p[r["car_idx"], :3],
                car_rgb=colors[f][r["car_mask"]] if len(r["car_idx"]) else np.zeros((0, 3)), bg_idx=r["bg_idx"], bg_xyz=p[r["bg_idx"], :3])


def check_first_match(got, ref, frames, colors, what, poison):
    """lpf_first_match's outputs against the reference; poison: the per-point outputs were handed over poisoned (device memory) and
    must still hold the poison at and beyond each frame's count"""
    off, F = ref["off"], len(frames)
    for f in range(F):
        a, b = int(off[f]), int(off[f + 1])
        rows = first_match_rows(ref, frames, colors, f)
        nc, nb = len(rows["car_idx"]), len(rows["bg_idx"])
        assert int(got["n_car"][f]) == nc and int(got["n_bg"][f]) == nb and int(got["n_valid"][f]) == nc + nb, (what, f, "counts")
        assert np.array_equal(np.asarray(got["mask_count"]).reshape(F, -1)[f], ref["per"][f]["mask_count"]), (what, f, "mask_count")
        for k, want in rows.items():
            if b == a:
                continue
            n = len(want)
            g = np.asarray(got[k])[a:a + n]
            assert g.tobytes() == np.ascontiguousarray(want, g.dtype).tobytes(), (what, f, k)
            if poison and k != "first_mask":
                assert _intact(np.asarray(got[k])[a + n:b]), (what, f, k, "written beyond the frame's count")


def forge_first_match(ref, frames, colors):
    Ntot, F = int(ref["off"][-1]), len(frames)
    h = {k: poisoned((Ntot,) + tail, dt) for k, (tail, dt) in FM_SHAPES.items()}
    h.update(n_valid=np.zeros(F, np.int64), n_car=np.zeros(F, np.int64), n_bg=np.zeros(F, np.int64), mask_count=np.zeros((F, ref["M"]), np.int64))
    for f in range(F):
        a = int(ref["off"][f])
        rows = first_match_rows(ref, frames, colors, f)
        for k, want in rows.items():
            h[k][a:a + len(want)] = want
        nc, nb = len(rows["car_idx"]), len(rows["bg_idx"])
        h["n_car"][f], h["n_bg"][f], h["n_valid"][f], h["mask_count"][f] = nc, nb, nc + nb, ref["per"][f]["mask_count"]
    return h


def check_wide(op, res, refs, what):
    assert len(res) == len(refs), (what, "frames")
    for f in range(len(refs)):
        try:
            WG.compare(res[f], refs[f], (what, f))
        except AssertionError as e:
            raise AssertionError((what,) + tuple(e.args)) from None


def check_maps(got, want, what):
    from test_gpu_depth_maps import _same
    assert len(got) == len(want), (what, "frames")
    for f in range(len(want)):
        _same(got[f], want[f], (what, f))


def check_bits(got, ref, what):
    why = BR.compare(got, ref)
    assert why is None, (what, why)
