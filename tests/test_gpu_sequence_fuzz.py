"""Model-based sequence fuzz: every seed's 10 to 14 calls of tests/sequence_fuzz_cases.py on ONE LpfContext that starts in order, under
"fused" and under "fused-pack", every output compared bit for bit with the reference for the state the model says is in force -- the
last narrow run issued again with nothing set again that include/lpf.h lets stand, directly behind every wide, multi-camera and
analysis call; camera sizes that shrink and grow; mask counts down and up across 32; the erosion element changed between a pack and
its rerun; mode switches with work owed; the documented refusals of a pipelined run without its masks and of a call on boxes that were cleared; once more on the lab
library with the range limits and the launch geometry changed between the ops.  Device outputs are handed over
filled with 0xA5 and must still hold it where the header says nothing is written.  Lent inputs and all outputs stay alive and
untouched until the final sync(); every comparison happens after it.  What the default seeds reach is asserted on the CPU
(tests/test_sequence_fuzz_cases.py).  LPF_FUZZ_CASES and LPF_FUZZ_SEED_BASE choose other seeds, as in tests/test_gpu_fuzz.py."""
import functools

import numpy as np
import pytest

import batch_range_cases as BR
import box_views_ref as BV
import narrow_fuzz_cases as NG
import sequence_fuzz_cases as G
import wide_fuzz_cases as WG
from conftest import load_calib
from test_gpu_batch_ranges import run as run_pairs
from test_gpu_fuzz_narrow import _dev, _set_boxes, _unaligned

pytestmark = pytest.mark.gpu

SEEDS = G.seeds()


@functools.lru_cache(maxsize=2)
def _sequence(seed):
    return G.sequence(seed, load_calib())


@functools.lru_cache(maxsize=2)
def _expectations(seed, mode):
    """the seed's expectations from a context that starts in ``mode``: shared by the tests of (seed, mode) and left unchanged"""
    return G.expectations(_sequence(seed), mode)


def _poisoned(shape, dtype):
    import torch
    t = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
    t.view(torch.uint8).fill_(G.POISON)
    return t


def _set_masks(ctx, cs, refs, source, keep):
    """the case's masks (and rectangles) from ``source``, WITHOUT touching the erosion element: it is the one in force"""
    M = cs["M"]
    if source == "label":
        ctx.set_label_image(np.stack([r["label_img"] for r in refs]), M)
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


def _narrow_op(ctx, e, keep):
    """a narrow run or rerun: the set-up calls the model lists, then the run on its route; returns what _finish reads"""
    import torch
    from lidar_object_detection_amd._native import LpfError
    cs, refs, route = e["case"], e["refs"], e["route"]
    fl = NG.fields(cs)
    cap, tight = G.capacity(cs, refs)
    if "camera" in e["setup"]:
        ctx.set_camera(cs["T"], cs["K"], cs["W"], cs["H"], cs["dmin"], cs["dmax"])
    if route == "host":
        _set_masks(ctx, cs, refs, e["source"], keep)
        vis = _set_boxes(ctx, cs, refs, keep, device=False)
        got = ctx.run_batch(cs["frames"], want_uv="uv" in fl, want_label="label_bits" in fl, want_float=cs["want_float"],
                            want_lists="inst_idx" in fl, want_valid_uv="uv_valid" in fl, inst_cap=cap if tight else None)
        for f, r in enumerate(got):
            r.pop("uv_valid", None)
            if vis is not None:
                r["visible"] = vis[f]
        return dict(host=got)
    n = int(sum(cs["sizes"]))
    off = np.concatenate([[0], np.cumsum(cs["sizes"])]).astype(np.int64)
    pts = _dev(np.concatenate(cs["frames"]).reshape(-1, 4)) if n else torch.zeros((1, 4), dtype=torch.float32, device="cuda")
    o = {k: _poisoned(*sd) for k, sd in G.narrow_shapes(cs, fl, cap).items()}
    keep.append(pts)
    kw = dict(o, inst_cap=cap) if "inst_idx" in o else dict(o)
    vis = None
    if route == "step":
        B = len(cs["cam0"][0])
        masks, cam0 = _dev(cs["masks"][0]), _dev(cs["cam0"][0])
        rects = _dev(cs["rects"][0]) if cs["rects"] is not None else None
        keep += [masks, cam0, rects]
        torch.cuda.synchronize()
        if B == 0:
            ctx.clear_boxes()
        step = ctx.make_frame_step(pts, masks_u8=masks, mask_rects=rects, boxes_cam0=cam0 if B else None, T_cam_to_velo=cs["Tcv"],
                                   filter_visible=cs["box_source"] == "cam0-visible", oriented=cs["oriented"], **kw)
        keep.append(step)
        step()
        return dict(dev=o, cap=cap)
    torch.cuda.synchronize()
    if "masks" in e["setup"]:
        _set_masks(ctx, cs, refs, e["source"], keep)
    if "boxes" in e["setup"]:
        vis = _set_boxes(ctx, cs, refs, keep, device=True)
    if route == "step-null":                                  # NULL masks, NULL corners: both stay in force (include/lpf.h, lpf_run_frame)
        step = ctx.make_frame_step(pts, **kw)
        keep.append(step)
        step()
        return dict(dev=o, cap=cap)
    if e["refuse"]:
        with pytest.raises(LpfError) as err:
            ctx.run_device(pts, off, **kw)
        return dict(refused=str(err.value))
    ctx.run_device(pts, off, **kw)
    return dict(dev=o, cap=cap, vis=vis)


def _cams_specs(op, frames):
    specs = []
    for k, cam in enumerate(op["case"]["cams"]):
        dev = (op["case"]["seed"] + k) % 2 == 1
        masks, rects = cam["masks"], cam["rects"]
        specs.append(dict(T_velo_to_rect=cam["T"], K=cam["K"], width=cam["W"], height=cam["H"], depth_min=cam["dmin"], depth_max=cam["dmax"],
                          masks=_dev(masks) if dev else masks, rects=(_dev(rects) if dev else rects) if rects is not None else None,
                          binarize=cam["binarize"], erode_iters=cam["erode"], boxes=cam["boxes"], oriented=cam["oriented"]))
    return specs


def _run_op(ctx, op, e, keep, last=None):
    """one op on the context; returns the record _finish compares once everything has been synchronised.  last: the device outputs of
    the most recent narrow run, still being written when the pipeline owes work"""
    import torch
    kind = op["kind"]
    if kind in ("narrow", "rerun", "rerun-unset"):
        return _narrow_op(ctx, e, keep)
    if kind == "set_element":
        ctx.set_erosion_element(op["k"])
    elif kind == "set_pipelined":
        ctx.set_pipelined(False if e["mode"] == "off" else e["mode"])
    elif kind == "sync":
        ctx.sync()
    elif kind == "label":
        if "pipelined-off" in e["setup"]:
            ctx.set_pipelined(False)
        if "masks" in e["setup"]:
            _set_masks(ctx, e["case"], e["refs"], e["source"], keep)
        return dict(label=ctx.get_label_image())
    elif kind == "wide":
        cam = op["cam"]
        masks, rects = cam["masks"], cam["rects"]
        if op["device"]:
            masks, rects = _dev(masks), (_dev(rects) if rects is not None else None)
        keep += [masks, rects]
        return dict(res=ctx.run_wide(e["frames"], masks, erode_iters=cam["erode"], binarize=cam["binarize"], rects=rects, want_float=True,
                                     want_valid_uv=True))
    elif kind == "cams":
        specs = _cams_specs(op, e["frames"])
        keep.append(specs)
        call = ctx.run_cams_wide if op["wide"] else ctx.run_cams
        return dict(res=call(e["frames"], specs, want_float=True, want_valid_uv=True))
    elif kind == "first_match":
        masks, colors, out = op["masks"], op["colors"], None
        Ntot = int(e["ref"]["off"][-1])
        if op["device"]:
            masks, colors = _dev(masks), _dev(colors)
            if Ntot:
                out = {k: _poisoned((Ntot,) + tail, dt) for k, (tail, dt) in G.FM_SHAPES.items()}
            dims = dict(F=masks.shape[0], M=masks.shape[1])
            out = dict(out or {}, **{k: _poisoned(tuple(dims[d] for d in sh), np.int64) for k, sh in G.FM_PER_FRAME.items()})
            torch.cuda.synchronize()
        keep += [masks, colors, out]
        return dict(res=ctx.first_match(e["frames"], masks, colors, out=out), poison=bool(op["device"] and Ntot))
    elif kind == "depth_maps":
        cam = op["cam"]
        masks, rects = cam["masks"], cam["rects"]
        if op["device"]:
            masks, rects = _dev(masks), (_dev(rects) if rects is not None else None)
        full = np.ones(np.shape(cam["masks"]), np.uint8)
        full = _dev(full) if op["device"] else full
        keep += [masks, rects, full]
        primer = ctx.depth_maps(e["frames"], full, binarize="astype")
        if op["device"] and sum(len(p) for p in e["frames"]):
            return dict(maps_dev=_depth_maps_device(ctx, e["frames"], cam, masks, rects, e["dev_cap"], keep), cap=e["dev_cap"], primer=primer)
        return dict(maps=ctx.depth_maps(e["frames"], masks, binarize=cam["binarize"], rects=rects, erode_iters=cam["erode"], cap=op["cap"]),
                    primer=primer)
    elif kind == "pairs":
        return dict(bits=run_pairs(ctx, BR.case(op["call"]), op["place"], setup=False))
    elif kind in ("inside_masks", "box_points"):
        from lidar_object_detection_amd._native import LpfError
        dev = op["device"]
        if e["refuse"]:
            F = len(e["frames"])
            empty = [np.zeros((F, 1), np.int64), np.zeros((F, 1), np.int64), np.zeros((F, 0), np.int32), np.zeros((F, 0), np.int64)]
            with pytest.raises((LpfError, ValueError)) as err:
                if kind == "inside_masks":
                    ctx.inside_masks(e["frames"], *empty)
                else:
                    n = sum(len(p) for p in e["frames"])
                    ctx.box_points(e["frames"], np.zeros(n, np.int64), np.zeros(F, np.int64))
            return dict(refused=str(err.value))
        I = e["inputs"]
        put = _dev if dev else (lambda a: a)
        if kind == "inside_masks":
            F, M, cap = len(e["frames"]), I["best_box"].shape[1], e["cap"]
            lists = [put(I[k]) for k in ("inst_idx", "inst_off", "best_box", "best_cnt")]
            out = dict(inside=_poisoned((F, cap), np.uint8), part_idx=_poisoned((F, cap), np.int64), part_xyz=_poisoned((F, cap, 3), np.float32),
                       n_inside=_poisoned((F, M), np.int64), matched=_poisoned((F, M), np.int32)) if dev else None
            torch.cuda.synchronize()
            keep += [lists, out]
            return dict(inside=ctx.inside_masks(e["frames"], *lists, min_points=G.MIN_POINTS, out=out), poison=dev)
        lists = [put(I["valid_idx"]), put(I["n_valid"]), put(I["label_valid"].view(np.int32))]
        if dev and last is not None and len(I["valid_idx"]):
            # the run's OWN compact lists, as it wrote (or is still to write) them on the device: nothing is waited for in between, so
            # the call has to come behind the run's tail by itself (the counts per frame are the reference's)
            lists = [last["valid_idx"], lists[1], last["label_valid"]]
        out = dict(first_box=_poisoned((len(I["valid_idx"]),), np.int32)) if (dev and len(I["valid_idx"])) else None
        torch.cuda.synchronize()
        keep += [lists, out]
        return dict(boxpts=ctx.box_points(e["frames"], *lists, out=out), poison=out is not None)
    elif kind == "operators":
        pts = e["frames"][e["frame"]]
        D, win = ctx.depth_image(pts)
        got = dict(D=D, win=win, visible=ctx.prepare_boxes(e["cam0"], e["Tcv"])[0], inside=ctx.points_in_boxes(pts[:200], e["velo"], e["oriented"]))
        planes, small = (_dev(op["planes"]), _dev(op["small"])) if op["device"] else (op["planes"], op["small"])
        keep += [planes, small]
        got.update(eroded=ctx.erode_masks(planes, op["iters"]), resized=ctx.resize_masks(small))
        return dict(operators=got)
    elif kind == "clear_boxes":
        from lidar_object_detection_amd._native import LpfError
        ctx.clear_boxes()
        F = len(e["frames"])
        n = sum(len(p) for p in e["frames"])
        empty = [np.zeros((F, 1), np.int64), np.zeros((F, 1), np.int64), np.zeros((F, 0), np.int32), np.zeros((F, 0), np.int64)]
        return dict(refused=_refused((LpfError, ValueError), lambda: ctx.inside_masks(e["frames"], *empty)),
                    refused2=_refused((LpfError, ValueError), lambda: ctx.box_points(e["frames"], np.zeros(n, np.int64), np.zeros(F, np.int64))))
    elif kind == "frame_wide":
        from lidar_object_detection_amd._native import LpfError
        from test_gpu_frame_wide import _outs
        cam, pts = op["cam"], e["pts"]
        dp, dm = _dev(pts) if len(pts) else torch.zeros((0, 4), dtype=torch.float32, device="cuda"), _dev(np.ascontiguousarray(cam["member"][0], np.uint8))
        dr = _dev(cam["fw_rects"]["hold"][0]) if op["rects"] else None
        cap = 1 if e["refuse"] else e["cap"]
        o = _outs(len(pts), cam["M"], 0 if e["refuse"] else e["B"], cap)             # (filled with 0xA5)
        step = ctx.make_frame_step_wide(dp, dm, mask_rects=dr, inst_cap=cap, **o)     # NULL corners: the boxes in force
        keep += [dp, dm, dr, o, step]
        torch.cuda.synchronize()
        if e["refuse"]:
            return dict(refused=_refused(LpfError, step))
        step()
        return dict(frame_wide=o)
    elif kind == "depth_overlays":
        from lidar_object_detection_amd._native import LpfError
        cam = op["cam"]
        maps = ctx.depth_maps(e["frames"], cam["masks"], binarize=cam["binarize"], rects=cam["rects"], erode_iters=cam["erode"])
        if e["refuse"]:
            return dict(maps=maps, primer=None, refused=_refused((LpfError, ValueError), lambda: ctx.depth_overlays(maps, op["seg"])))
        seg = _dev(op["seg"]) if op["device"] else op["seg"]
        keep.append(seg)
        images, mx = ctx.depth_overlays(maps, seg)
        return dict(maps=maps, primer=None, overlays=dict(images=images, max_depth=mx))
    elif kind == "box_views":
        corners = _dev(op["corners"]) if op["device"] else op["corners"]
        keep.append(corners)
        return dict(views=ctx.box_views(corners, op["box_off"], op["Tcv"], want=BV.WANT))
    else:
        raise KeyError(kind)
    return {}


def _depth_maps_device(ctx, frames, cam, masks, rects, cap, keep):
    """lpf_depth_maps with the masks and every output in device memory, the outputs poisoned (LpfContext.depth_maps' out=): one call,
    nothing read back"""
    import torch
    outs = {k: _poisoned(*sd) for k, sd in G.maps_shapes(len(frames), cam["M"], cap).items()}
    keep.append(outs)
    torch.cuda.synchronize()
    return ctx.depth_maps(frames, masks, binarize=cam["binarize"], rects=rects, erode_iters=cam["erode"], cap=cap, out=outs)


def _refused(what_raises, call):
    """the message of the refusal ``call`` has to end in"""
    with pytest.raises(what_raises) as err:
        call()
    return str(err.value)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _finish(seq, exps, recs, mode):
    """Every record against its expectation; returns, per op, the bytes of everything the op wrote or was to leave alone (the rows of
    frames whose instance lists did not fit left out: include/lpf.h does not say what a truncated list holds)."""
    snap = []
    for i, (op, e, rec) in enumerate(zip(seq.ops, exps, recs)):
        what = ("seed %d" % seq.seed, mode, "op %d" % i, op["kind"])
        s = {}
        if e["refuse"]:
            assert e["refuse"] in rec["refused"] and e["refuse"] in rec.get("refused2", rec["refused"]), (what, rec)
            if "maps" in rec:
                G.check_maps(rec["maps"], e["maps"], what)
        elif "host" in rec:
            try:
                NG.check(e["case"], rec["host"], e["refs"], route=str(what))
            except AssertionError as err:
                raise AssertionError((what,) + tuple(err.args)) from None
            s = {"%d.%s" % (f, k): np.asarray(v) for f, r in enumerate(rec["host"]) for k, v in r.items() if k != "inst_lists"}
        elif "dev" in rec:
            h = {k: t.cpu().numpy() for k, t in rec["dev"].items()}
            vis = rec.get("vis")
            visible = None
            if vis is not None:
                v, boff = vis[0].cpu().numpy(), vis[1]
                visible = [v[int(boff[f]):int(boff[f + 1])] for f in range(len(boff) - 1)]
            G.check_narrow(e["case"], h, e["refs"], rec["cap"], what, visible)
            s = dict(h)
            if "inst_idx" in s:
                s["inst_idx"] = s["inst_idx"].copy()
                for f, r in enumerate(e["refs"]):
                    if r["need"] > rec["cap"]:
                        s["inst_idx"][f] = 0
        elif "label" in rec:
            G.check_label(rec["label"], e["label"], what)
            s = dict(label=rec["label"])
        elif "frame_wide" in rec:
            h = {k: t.cpu().numpy() for k, t in rec["frame_wide"].items()}
            G.check_frame_wide(h, e["ref"], op["cam"]["M"], e["B"], what)
            s = h
        elif "maps_dev" in rec:
            h = {k: t.cpu().numpy() for k, t in rec["maps_dev"].items()}
            G.check_maps(rec["primer"], e["primer"], what + ("every mask full",))
            G.check_maps_device(h, e["maps"], rec["cap"], what)
            s = {k: v for k, v in h.items() if k in ("car_off", "need", "overflow")}
            for k in ("pix", "depth", "point_idx"):           # (the rows of the frames that fit, and the guard row)
                s[k] = np.where(np.append(h["need"] <= rec["cap"], True)[:, None], h[k], 0)
        elif "res" in rec and op["kind"] == "wide":
            G.check_wide(op, rec["res"], e["refs"], what)
        elif "res" in rec and op["kind"] == "cams":
            G.check_cams(op, rec["res"], e["refs"], what)
        elif "res" in rec:
            got = {k: _np(v) for k, v in rec["res"].items()}
            G.check_first_match(got, e["ref"], e["frames"], op["colors"], what, rec["poison"])
            s = got if rec["poison"] else {k: got[k] for k in ("n_valid", "n_car", "n_bg", "mask_count", "first_mask")}
        elif "maps" in rec:
            if rec["primer"] is not None:
                G.check_maps(rec["primer"], e["primer"], what + ("every mask full",))
            G.check_maps(rec["maps"], e["maps"], what)
            if "overlays" in rec:
                got = {k: _np(v) for k, v in rec["overlays"].items()}
                G.check_bits(got, e["ref"], what)
                s = got
        elif "bits" in rec:
            G.check_bits(rec["bits"], e["ref"], what)
            s = rec["bits"]
        elif "inside" in rec:
            got = {k: _np(v) for k, v in rec["inside"].items()}
            G.check_inside(got, e, what, rec["poison"])
            s = got
        elif "boxpts" in rec:
            got = {k: _np(v) for k, v in rec["boxpts"].items()}
            G.check_box_points(got, e, what, rec["poison"])
            s = got if rec["poison"] else {k: got[k] for k in ("box_points", "box_labelled", "frame_counts")}
        elif "operators" in rec:
            got = {k: _np(v) for k, v in rec["operators"].items()}
            G.check_operators(got, e["ref"], what)
            s = got
        elif "views" in rec:
            got = {k: _np(v) for k, v in rec["views"].items()}
            G.check_bits(got, e["ref"], what)
            s = got
        snap.append({k: np.ascontiguousarray(v).tobytes() for k, v in s.items()})
    return snap


def _one_pass(ctx, seq, mode, lab=False):
    """the sequence on ``ctx`` from ``mode`` and the 3 x 3 element: everything queued, ONE sync, then every comparison.  lab: the
    range limits, and where nothing is owed the launch geometry, are changed before every op (sequence_fuzz_cases.lab_settings)"""
    import torch
    exps = _expectations(seq.seed, mode)
    ctx.set_pipelined(False if mode == "off" else mode)
    ctx.set_erosion_element(3)
    keep, recs, last = [], [], None
    for i, (op, e) in enumerate(zip(seq.ops, exps)):
        if lab:
            form, budget, most = G.lab_settings(seq.seed, i, e["idle"])
            if form is not None:
                ctx.set_geometry(form)
            ctx.set_range_limits(budget, most)
        try:
            recs.append(_run_op(ctx, op, e, keep, last))
            if op["kind"] in ("narrow", "rerun"):
                last = recs[-1].get("dev")
        except (Exception, pytest.fail.Exception) as err:   # (a set-up call that raises, a refusal that does not come)
            raise AssertionError(("seed %d" % seq.seed, mode, "op %d" % i, op["kind"], "%s: %s" % (type(err).__name__, err))) from err
    ctx.sync()
    torch.cuda.synchronize()
    return _finish(seq, exps, recs, mode)


@pytest.mark.parametrize("mode", G.MODES)
@pytest.mark.parametrize("seed", SEEDS)
def test_sequence(seed, mode):
    """the seed's sequence on a fresh context that starts in ``mode``"""
    from lidar_object_detection_amd._native import LpfContext
    with LpfContext(0) as ctx:
        _one_pass(ctx, _sequence(seed), mode)


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_under_lab_settings(seed):
    """the seed's sequence on a context of the lab library, from mode seed % 3, with lpf_lab_set_range_limits before every op and
    lpf_set_geometry before every op that finds nothing owed: results do not depend on either (include/lpf.h)"""
    from conftest import lab_library
    from lidar_object_detection_amd._native import LpfContext
    path = lab_library()
    if path is None:
        pytest.skip("liblpf_lab.so has not been built (python -m lidar_object_detection_amd._build lab)")
    with LpfContext(0, library=path) as ctx:
        _one_pass(ctx, _sequence(seed), G.MODES[seed % 3], lab=True)


@pytest.mark.parametrize("mode", G.MODES)
@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_twice_on_one_context(seed, mode):
    """The sequence twice on one context (the second pass starts from what the first left behind, with the mode and the element
    put back): both passes hold against the references, and the second gives the same bytes as the first, poisoned regions
    included."""
    from lidar_object_detection_amd._native import LpfContext
    seq = _sequence(seed)
    with LpfContext(0) as ctx:
        first = _one_pass(ctx, seq, mode)
        second = _one_pass(ctx, seq, mode)
    for i, (a, b) in enumerate(zip(first, second)):
        assert a.keys() == b.keys(), (seed, mode, i, seq.ops[i]["kind"])
        for k in a:
            assert a[k] == b[k], ("seed %d" % seed, mode, "op %d" % i, seq.ops[i]["kind"], k, "the second pass differs from the first")
