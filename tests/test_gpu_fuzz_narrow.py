"""Seeded differential fuzz of the narrow path -- lpf_run_batch in order and software-pipelined, lpf_run_frame, the step kernel under
every launch geometry and the three mask packs -- against the C oracle, bit for bit in every output asked for.  The cases come from
tests/narrow_fuzz_cases.py: eight camera sizes (hw odd; hw % 16 == 0 with W % 16 != 0, where the streaming pack's groups straddle
rows; W < 16, where the rectangle hint is dropped), depth_min of 0, 0.5 and -5 with a point exactly on it, every label width out of
the streaming and the tiled pack, uint8 and float masks under the three rules, erosion by the 3 x 3 and the 5 x 5 element, masks from
host memory, copied or lent device tensors, a lent tensor that is not 16-byte aligned and a label image handed over
(lpf_set_label_image), rectangles that hold and that do not, boxes from velodyne or cam-0 corners with and without the visibility
filter, and subsets of the outputs.  What the default seeds reach is asserted on the CPU (tests/test_narrow_fuzz_cases.py).
LPF_FUZZ_CASES and LPF_FUZZ_SEED_BASE choose other seeds, as in tests/test_gpu_fuzz.py."""
import functools

import numpy as np
import pytest

import narrow_fuzz_cases as G
from conftest import load_calib

pytestmark = pytest.mark.gpu

SEEDS = G.seeds()
GROUPS = range((len(SEEDS) + 2) // 3)                         # three consecutive cases per pipelined context


def _steps(seed):
    """lpf_run_frame takes uint8 masks as they are: the cases without erosion that have masks and frames with points"""
    p = G.plan(seed)
    return p["kind"] == "u8" and p["erode"] == 0 and p["M"] > 0 and p["layout"] not in ("all", "single")


STEP_SEEDS = [s for s in SEEDS if _steps(s)]


@functools.lru_cache(maxsize=4)
def _fuzz(seed):
    """the seed's case and its oracle results, shared by the tests that follow each other on the seed and left unchanged"""
    cs = G.case(seed, load_calib())
    return cs, G.reference(cs)


def _capacity(cs, refs):
    """(inst_cap, tight): room for the frame that needs most, or -- odd seeds -- less than that, so that it overflows next to frames
    that fit"""
    cap = G.tight_inst_cap(refs) if cs["tight_cap"] else None
    return (cap, True) if cap is not None else (max(max(r["need"] for r in refs), 1), False)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _unaligned(a):
    """the array in a GPU buffer one element longer, viewed from element 1: 1 byte (uint8) or 4 bytes (float32) past a 16-byte
    boundary"""
    import torch
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0].reshape(-1)).dtype, device="cuda")
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == a.itemsize and view.is_contiguous()
    return view


def _set_masks(ctx, cs, refs, source, keep):
    """the case's masks (and rectangles) from ``source``; keep: what must stay alive and unchanged until the run is complete"""
    M, F = cs["M"], cs["F"]
    ctx.set_erosion_element(cs["element"])
    if source == "label":
        want = np.stack([r["label_img"] for r in refs])
        ctx.set_label_image(want, M)
        assert np.array_equal(ctx.get_label_image(), want), (cs["seed"], "label image read back")
        return
    if M == 0:
        ctx.clear_masks()
        return
    lent = source.startswith("lent")
    if cs["rects"] is not None:
        rects = _dev(cs["rects"]) if lent else cs["rects"]
        keep.append(rects)
        ctx.set_mask_rects(rects)
    masks = cs["masks"] if source == "host" else _unaligned(cs["masks"]) if source == "lent-unaligned" else _dev(cs["masks"])
    keep.append(masks)
    ctx.set_masks(masks, erode_iters=cs["erode"], binarize=cs["binarize"], lend=lent)


def _set_boxes(ctx, cs, refs, keep, device):
    """the case's boxes from its source; returns the ``visible`` output (per frame) under "cam0-visible", else None.  device: cam-0
    corners as a lent GPU tensor (nothing waits), else from host memory."""
    import torch
    src = cs["box_source"]
    boff = np.concatenate([[0], np.cumsum([len(c) for c in cs["cam0"]])]).astype(np.int32)
    if src.startswith("velo"):
        velo = [r["corners_velo"] for r in refs]
        if src == "velo-host":
            ctx.set_boxes(velo, oriented=cs["oriented"])
        else:
            t = _dev(np.concatenate(velo).reshape(-1, 8, 3))
            keep.append(t)
            ctx.set_boxes_device(t, boff, oriented=cs["oriented"], lend=True)
        return None
    filt = src == "cam0-visible"
    if not device:
        out = ctx.set_boxes_cam0(cs["cam0"], cs["Tcv"], filter_visible=filt, oriented=cs["oriented"])
        return [o[0] for o in out] if filt else None
    t = _dev(np.concatenate(cs["cam0"]).reshape(-1, 8, 3))
    vis = torch.zeros(max(int(boff[-1]), 1), dtype=torch.uint8, device="cuda")
    keep += [t, vis]
    ctx.set_boxes_cam0_device(t, boff, cs["Tcv"], filter_visible=filt, oriented=cs["oriented"], lend=True, visible=vis)
    return (vis, boff) if filt else None


# ---- serial routes: run_batch, host outputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["auto", "small-narrow", "small-1024", "large", "large-scan"])
@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_serial(seed, form):
    """run_batch in order, on the product library and under every forced launch geometry of the lab build, every mask source
    included.  The output subset goes through run_batch's want_* flags: "no-inst_idx" is want_lists=False (no valid_idx either),
    count_mb always comes back -- the pipelined routes ask for the exact subsets.  Odd seeds: an inst_cap below the largest frame's
    need; run_batch sees the overflow flag and runs once more with the exact capacity, so every list is compared."""
    from conftest import context_for_form
    cs, refs = _fuzz(seed)
    fl = G.fields(cs)
    cap, tight = _capacity(cs, refs)
    keep = []
    with context_for_form(form) as ctx:
        ctx.set_camera(cs["T"], cs["K"], cs["W"], cs["H"], cs["dmin"], cs["dmax"])
        _set_masks(ctx, cs, refs, cs["source"], keep)
        vis = _set_boxes(ctx, cs, refs, keep, device=False)
        got = ctx.run_batch(cs["frames"], want_uv="uv" in fl, want_label="label_bits" in fl, want_float=cs["want_float"],
                            want_lists="inst_idx" in fl, want_valid_uv="uv_valid" in fl, inst_cap=cap if tight else None)
    for f, r in enumerate(got):
        r.pop("uv_valid", None)                               # (u_valid, v_valid are its columns)
        if vis is not None:
            r["visible"] = vis[f]
    assert all(("u" in r) == ("uv" in fl) and ("label_bits" in r) == ("label_bits" in fl) and ("inst_lists" in r) == ("inst_idx" in fl)
               and ("depth" in r) == cs["want_float"] and "count_mb" in r for r in got), (seed, form)
    G.check(cs, got, refs, route=form)


# ---- device outputs: run_device, lpf_run_frame ------------------------------------------------------------------------------------------
def _outputs(cs, sizes, Btot, fl, cap):
    """preallocated GPU tensors for the fields ``fl`` of a run over frames of ``sizes`` points"""
    import torch
    from lidar_object_detection_amd._native import SUMMARY_DTYPE
    n, F, M = max(int(sum(sizes)), 1), len(sizes), cs["M"]
    shapes = dict(uv=((n, 2), torch.int32), label_bits=((n,), torch.int32), depth=((n,), torch.float64), u_f=((n,), torch.float64),
                  v_f=((n,), torch.float64), valid_idx=((n,), torch.int64), inst_idx=((F, cap), torch.int64),
                  count_mb=((max(M * Btot, 1),), torch.int32), uv_valid=((n, 2), torch.int32), label_valid=((n,), torch.int32))
    o = {k: torch.full(shapes[k][0], -7, dtype=shapes[k][1], device="cuda") for k in fl}
    if "count_mb" in o:
        o["count_mb"].zero_()
    o["summary"] = torch.zeros(F * SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    if "inst_idx" in fl:
        o["inst_cap"] = cap
    return o


def _read(cs, o, sizes, box_counts, vis=None):
    """the device outputs of a run as one dict per frame, keys as run_batch names them"""
    from lidar_object_detection_amd._native import SUMMARY_DTYPE
    M = cs["M"]
    h = {k: t.cpu().numpy() for k, t in o.items() if k != "inst_cap"}
    sm = np.frombuffer(h["summary"].tobytes(), SUMMARY_DTYPE)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    boff = np.concatenate([[0], np.cumsum(box_counts)]).astype(np.int64)
    got = []
    for f in range(len(sizes)):
        a, b, s = int(off[f]), int(off[f + 1]), sm[f]
        nv = int(s["n_valid"])
        assert 0 <= nv <= b - a, (cs["seed"], f, "n_valid", nv)
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
            B = int(box_counts[f])
            r["count_mb"] = h["count_mb"][M * int(boff[f]):M * int(boff[f + 1])].reshape(M, B)
        if vis is not None:
            r["visible"] = vis[0].cpu().numpy()[int(vis[1][f]):int(vis[1][f + 1])]
        got.append(r)
    return got


def _queue(ctx, cs, refs):
    """One run_device of the case on ``ctx`` -- camera, masks, boxes, then the run, nothing waited for after the inputs are on the GPU;
    returns what _check_queued reads once the context has been synchronised (and what must live until then)."""
    import torch
    fl = G.fields(cs)
    cap, _ = _capacity(cs, refs)
    n = int(sum(cs["sizes"]))
    off = np.concatenate([[0], np.cumsum(cs["sizes"])]).astype(np.int64)
    pts = _dev(np.concatenate(cs["frames"]).reshape(-1, 4)) if n else torch.zeros((1, 4), dtype=torch.float32, device="cuda")
    o = _outputs(cs, cs["sizes"], sum(len(c) for c in cs["cam0"]), fl, cap)
    keep = [pts]
    torch.cuda.synchronize()
    ctx.set_camera(cs["T"], cs["K"], cs["W"], cs["H"], cs["dmin"], cs["dmax"])
    _set_masks(ctx, cs, refs, "lent" if cs["source"] == "label" else cs["source"], keep)
    vis = _set_boxes(ctx, cs, refs, keep, device=True)
    ctx.run_device(pts, off, **o)
    return o, vis, cap, keep


def _check_queued(cs, refs, held, route):
    o, vis, cap, _ = held
    got = _read(cs, o, cs["sizes"], [len(c) for c in cs["cam0"]], vis)
    G.check(cs, got, refs, route=route, inst_cap=cap if "inst_idx" in o else None)


MODES = ["off", "fused", "fused-pack", "off+large", "fused+large", "fused-pack+large"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", GROUPS)
def test_fuzz_device_mode(seed, mode):
    """run_device in order and under lpf_set_pipelined(2 / 4), each also with the large launch geometry forced (lab build): three
    consecutive cases per context with nothing synchronised in between -- another camera size (lpf_set_camera lands between
    pipelined runs), depth window, erosion element, masks, rectangles and boxes from one run to the next -- and exactly the case's
    output subset, the other pointers NULL.  Odd seeds run with an inst_cap that the largest frame overflows: its inst_overflow is 1
    and its lists are not compared (include/lpf.h does not say what a truncated list holds); everything else is, and the frames
    that fit are compared in full.  A case whose mask source is the label image lends its masks instead: lpf_set_label_image drains
    the pipeline, and masks that a pipelined lpf_set_masks_* left unpacked win over it (its comment in lpf_api.hip)."""
    from conftest import context_for_form
    group = [_fuzz(SEEDS[(3 * seed + j) % len(SEEDS)]) for j in range(3)]
    held = []
    with context_for_form("large" if "+large" in mode else "auto") as ctx:
        pipe = mode.split("+")[0]
        ctx.set_pipelined(False if pipe == "off" else pipe)
        for cs, refs in group:
            held.append(_queue(ctx, cs, refs))
        ctx.sync()
    for (cs, refs), h in zip(group, held):
        _check_queued(cs, refs, h, mode)


@pytest.mark.parametrize("mode", ["fused", "fused-pack"])
def test_host_masks_before_every_pipelined_run(mode):
    """Regression, found by test_fuzz_device_mode[0-fused] on seed 4002: masks in HOST memory set before every run of a pipelined
    stream, as include/lpf.h asks.  lpf_set_masks_* left their label image in scratch set 0 whatever set the next run took, so every
    run but the first after a mode switch was refused ("the masks were set for another scratch set").  Five runs of the case: every
    set of the rotation of three (mode 2) and of four (mode 4) and the first one again."""
    from lidar_object_detection_amd._native import LpfContext
    cs, refs = _fuzz(G.DEFAULT_SEED_BASE + 2)
    assert cs["source"] == "host" and cs["M"] > 0
    with LpfContext(0) as ctx:
        ctx.set_pipelined(mode)
        held = [_queue(ctx, cs, refs) for _ in range(5)]
        ctx.sync()
    for k, h in enumerate(held):
        _check_queued(cs, refs, h, "%s, run %d" % (mode, k))


@pytest.mark.parametrize("mode", ["fused", "fused-pack"])
def test_queued_run_keeps_its_labels_when_the_next_run_brings_others(mode):
    """Regression, found by tests/test_gpu_sequence_fuzz.py on its seed 7054: a pipelined run that is asked for label_valid WITHOUT
    label_bits gathers its compact labels from dense ones of its own, which lived in ONE buffer of the context (narrow_bind), so the
    tiles of the next run overwrote them in the very launch in which this run's tail read them.  They now live in the run's scratch
    set.  The case as the fuzz met it, written out: row 10 of PLAN at 150 x 37 with 17 masks -- two frames of 0 and 65 points, float
    masks under "v3" with one erosion, lent from an unaligned tensor, outputs without label_bits -- run twice; lpf_box_points with host
    operands (it drains the pipeline); run again with the 3 x 3 element; then, with its masks set again under the 5 x 5 element, once
    more.  The boxes and the camera are set once.  The third run's label_valid of frame 1 came back as the fourth's in 2 of 16 entries."""
    import torch
    from lidar_object_detection_amd._native import LpfContext
    cs = G.case(G.DEFAULT_SEED_BASE + 10, load_calib(), size=(150, 37), M=17)
    assert (cs["sizes"], cs["kind"], cs["erode"], cs["element"], cs["source"], cs["outs"]) == ([0, 65], "v3", 1, 3, "lent-unaligned", "no-label_bits")
    cs5 = dict(cs, element=5)
    refs, refs5 = G.reference(cs), G.reference(cs5)
    assert not np.array_equal(refs[1]["label_valid"], refs5[1]["label_valid"])       # the two elements leave other labels
    fl = G.fields(cs)
    cap, _ = _capacity(cs, refs)
    off = np.concatenate([[0], np.cumsum(cs["sizes"])]).astype(np.int64)
    pts = _dev(np.concatenate(cs["frames"]).reshape(-1, 4))
    valid_idx, labels = np.zeros(int(off[-1]), np.int64), np.zeros(int(off[-1]), np.uint32)
    for f, r in enumerate(refs):
        valid_idx[off[f]:off[f] + r["n_valid"]], labels[off[f]:off[f] + r["n_valid"]] = r["valid_idx"], r["label_valid"]
    keep, held = [], []

    def run(case, rf, masks):
        if masks:
            _set_masks(ctx, case, rf, case["source"], keep)
        o = _outputs(case, case["sizes"], sum(len(c) for c in case["cam0"]), fl, cap)
        torch.cuda.synchronize()
        ctx.run_device(pts, off, **o)
        held.append((o, rf))

    with LpfContext(0) as ctx:
        ctx.set_pipelined(mode)
        ctx.set_camera(cs["T"], cs["K"], cs["W"], cs["H"], cs["dmin"], cs["dmax"])
        _set_masks(ctx, cs, refs, cs["source"], keep)
        vis = _set_boxes(ctx, cs, refs, keep, device=True)
        run(cs, refs, False)
        run(cs, refs, True)
        ctx.box_points(cs["frames"], valid_idx, np.array([r["n_valid"] for r in refs], np.int64), labels)
        run(cs, refs, True)
        run(cs5, refs5, True)
        ctx.sync()
    for k, (o, rf) in enumerate(held):
        got = _read(cs, o, cs["sizes"], [len(c) for c in cs["cam0"]], vis if k == 0 else None)
        G.check(cs, got, rf, route="%s, run %d" % (mode, k), inst_cap=cap if "inst_idx" in o else None)


@pytest.mark.parametrize("mode", ["off", "fused", "fused-pack"])
@pytest.mark.parametrize("seed", STEP_SEEDS)
def test_fuzz_frame_step(seed, mode):
    """Every non-empty frame of a case whose masks are uint8 without erosion as a stream of single frames through make_frame_step
    (lpf_run_frame): masks, rectangles and cam-0 boxes lent, the case's output subset, one sync() at the end.  A frame without
    boxes clears them first: NULL corners would leave the previous frame's in force (include/lpf.h)."""
    import torch
    from lidar_object_detection_amd._native import LpfContext
    cs, refs = _fuzz(seed)
    fl = G.fields(cs)
    cap, _ = _capacity(cs, refs)
    filt = cs["box_source"] == "cam0-visible"                 # (lpf_run_frame takes cam-0 corners only: the other sources keep every box)
    frames = [f for f in range(cs["F"]) if cs["sizes"][f]]
    held = []
    with LpfContext(0) as ctx:
        ctx.set_pipelined(False if mode == "off" else mode)
        ctx.set_camera(cs["T"], cs["K"], cs["W"], cs["H"], cs["dmin"], cs["dmax"])
        for f in frames:
            B = len(cs["cam0"][f])
            pts, masks, cam0 = _dev(cs["frames"][f]), _dev(cs["masks"][f]), _dev(cs["cam0"][f])
            rects = _dev(cs["rects"][f]) if cs["rects"] is not None else None
            o = _outputs(cs, [cs["sizes"][f]], B, fl, cap)
            torch.cuda.synchronize()
            if B == 0:
                ctx.clear_boxes()
            step = ctx.make_frame_step(pts, masks_u8=masks, mask_rects=rects, boxes_cam0=cam0 if B else None, T_cam_to_velo=cs["Tcv"],
                                       filter_visible=filt, oriented=cs["oriented"], **o)
            step()
            held.append((o, step, pts, masks, cam0, rects))
        ctx.sync()
    for f, h in zip(frames, held):
        got = _read(cs, h[0], [cs["sizes"][f]], [len(cs["cam0"][f])])
        G.check(cs, got, [refs[f]], route="frame-step %s, frame %d" % (mode, f), inst_cap=cap if "inst_idx" in h[0] else None)
