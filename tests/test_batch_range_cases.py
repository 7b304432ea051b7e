"""The batches of tests/batch_range_cases.py on the CPU: (a) their references equal the per-call restatements and the C oracle, (b)
neighbouring non-empty items have different reference outputs, so no cut position hides behind equal data, and (c) compare() has
teeth: the answer a wrong range base would give -- range 2's rows written from range 1's base on -- is rejected, for the per-item and
the per-frame outputs of every call and at every cut.  Conditions on the cases, not measurements: no GPU is involved."""
import numpy as np
import pytest

import assign_ref as A
import batch_range_cases as C
import box_points_ref as BP
import box_views_ref as BV
import inside_ref as IR
import match2d_ref as M2
from lidar_object_detection_amd import pipeline


def test_the_batches_have_the_asked_shape():
    assert 12 <= C.F <= 24 and 12 <= C.FD <= 24
    for shape in (C.SHAPES, list(zip(C.POINTS, C.BOXES))):
        rows = [a for a, _ in shape]
        assert rows[0] == 0 and rows[-1] == 0 and 0 in rows[1:-1]
    assert any(a[0] == 0 and a[1] > 0 and b[0] > 0 and b[1] == 0 for a, b in zip(C.SHAPES, C.SHAPES[1:]))     # no detections | no boxes
    cam = C.camera()
    assert all((cam["W"] * cam["H"]) % n for n in (16, 64, 1024))
    ov = C.depth_overlays()
    assert ov.items == C.FD * C.MD and all(cut % C.MD for cut in (5, ov.items - 1))       # cuts of 5 and items - 1 fall inside a frame
    for call in C.CALLS:
        assert C.compare({k: np.array(v) for k, v in C.case(call).ref.items()}, C.case(call).ref) is None


# ---- (a) the references are the restatements' -------------------------------------------------------------------------------------------
def test_match_2d_reference_equals_the_scalar_functions():
    c = C.match_2d()
    for f, (d, b, fr) in enumerate(zip(c.inputs["dets"], c.inputs["bbox2d"], c.inputs["front"])):
        if len(d) == 0 or len(b) == 0:
            continue
        exp = M2.scalar_scores(d, b, fr, pipeline.calculate_matching_score, pipeline.calculate_iou_2d)
        got = {k: c.rows(k, f).reshape(len(d), len(b)) for k in ("iou", "center", "size", "total", "cost")}
        M2.compare_scores(got, exp, ("frame", f))
        bb, bi = M2.best(got["iou"], C.MIN_IOU)
        assert np.array_equal(c.rows("best_box", f), bb) and M2.same_bits(c.rows("best_iou", f), bi)
    assert (c.ref["best_box"] >= 0).sum() >= 10 and (c.ref["iou"] > 0).sum() >= 40


def test_assign_references_equal_the_solver_restatement():
    c = C.assign_costs()
    for f, (m, fr) in enumerate(zip(c.inputs["costs"], c.inputs["front"])):
        col = c.rows("col_of_row", f)
        if m.shape[0] == 0 or not (fr > 0).any():
            assert c.ref["status"][f] == 0 and (col == -1).all()
            continue
        st, rows, cols = A.solve_front(m, fr)
        assert st == c.ref["status"][f] == C.STATUS.get(f, 0)
        assert np.array_equal(np.flatnonzero(col >= 0), rows) and np.array_equal(col[rows], cols), f
    assert sorted(set(c.ref["status"].tolist())) == [0, 1, 2]
    c2, m2 = C.assign_2d(), C.match_2d()
    assert not c2.ref["status"].any() and c2.ref["accepted"].sum() >= 5
    for f, (d, b, fr) in enumerate(zip(c2.inputs["dets"], c2.inputs["bbox2d"], c2.inputs["front"])):
        box = c2.rows("box_of_det", f)
        live = np.flatnonzero(fr > 0)
        if len(d) == 0 or len(live) == 0:
            assert (box == -1).all() and not c2.rows("total", f).any()
            continue
        cost = M2.score(d, b, fr, C.WEIGHTS)["cost"]
        st, rows, cols = A.solve(cost[:, live])
        assert st == 0 and np.array_equal(np.flatnonzero(box >= 0), rows) and np.array_equal(box[rows], live[cols]), f
        if f != 8:                                           # (frame 8's front differs from lpf_match_2d's case: every column dropped)
            tot = m2.rows("total", f).reshape(len(d), len(b))
            assert M2.same_bits(c2.rows("total", f)[rows], tot[rows, box[rows]])
    assert not (c2.inputs["front"][8] > 0).any() and (c2.rows("box_of_det", 8) == -1).all()


def test_inside_and_box_points_references_equal_the_restatements():
    c = C.inside_masks()
    cap, M = c.inputs["cap"], c.inputs["M"]
    over = 0
    for f, s in enumerate(c.splits):
        n = int(s["off"][-1])
        again = IR.frame_split(c.inputs["frames"][f], c.lists[f], c.inputs["corners"][f], C.MIN_POINTS, True)
        assert np.array_equal(again["inside"], s["inside"]) and np.array_equal(c.inputs["best_box"][f], s["best_box"])
        if n > cap:                                          # the lists did not fit: the rows keep the caller's bytes
            over += 1
            assert f == C.OVERFLOW_FRAME and (c.ref["inside"][f] == 9).all() and (c.ref["part_idx"][f] == -7).all() and (c.ref["part_xyz"][f] == 2.5).all()
            assert not c.ref["n_inside"][f].any() and np.array_equal(c.ref["matched"][f], s["matched"]) and s["matched"].any()
            continue
        assert np.array_equal(c.ref["inside"][f, :n], s["inside"]) and (c.ref["inside"][f, n:] == 9).all()
        assert np.array_equal(c.ref["part_idx"][f, :n], s["part_idx"]) and (c.ref["part_idx"][f, n:] == -7).all()
        for m in range(M):
            a, e = int(s["off"][m]), int(s["off"][m + 1])
            assert int(c.ref["inside"][f, a:e].sum()) == int(c.ref["n_inside"][f, m])
    assert over == 1 and C.OVERFLOW_FRAME >= 5 and c.ref["matched"].sum() >= 8
    b = C.box_points()
    for f, (p, vi) in enumerate(zip(b.inputs["frames"], b.valid)):
        r = BP.frame_box_points(p, vi, b.inputs["corners"][f], b.labelled[f], True)
        got = b.rows("first_box", f)
        assert np.array_equal(got[:len(vi)], r["first_box"]) and (got[len(vi):] == -5).all()
        assert np.array_equal(b.rows("box_points", f), r["box_points"]) and np.array_equal(b.ref["frame_counts"][f], r["frame_counts"])
        assert (b.inputs["label_valid"][int(b.spans["first_box"][f]):][:len(vi)] != 0).sum() == r["frame_counts"][2]
    assert (b.ref["frame_counts"][:, 3] > 0).sum() >= 5


def test_box_views_and_first_match_references_frame_by_frame():
    c = C.box_views()
    i = c.inputs
    for f in range(c.items):
        a, e = int(i["box_off"][f]), int(i["box_off"][f + 1])
        one = BV.views(i["corners"][a:e], [0, e - a], i["K"], i["W"], i["H"], i["T_cam_to_velo"])
        for k in BV.WANT:
            assert BV.same_bits(one[k].reshape(c.rows(k, f).shape), c.rows(k, f)), (f, k)
    assert c.ref["keep"].sum() >= 5 and len(set(c.ref["reason"].tolist())) >= 4
    m = C.first_match()
    for f, r in enumerate(m.per):
        assert m.ref["mask_count"][f].sum() == m.ref["n_car"][f] == len(r["car_idx"])
        assert m.ref["n_valid"][f] == (r["first_mask"] > -2).sum()
        n = int(m.ref["n_car"][f])
        assert (m.rows("car_idx", f)[n:] == -7).all() and (m.rows("car_rgb", f)[n:] == 3.5).all()
    assert (m.ref["mask_count"] > 0).sum() >= 15


def test_depth_images_equal_the_oracles_and_overlays_touch_only_their_lists():
    from oracle import cpu_oracle as orc
    cam, c = C.camera(), C.depth_maps()
    for f, p in enumerate(c.inputs["frames"]):
        D, win = C.depth_image(p, cam)
        if len(p):
            Do, wo = orc.depth_image(p, cam["T"], cam["K"], cam["W"], cam["H"], 0.0, C.DMAX)
            assert np.array_equal(D.view(np.int64), Do.view(np.int64)) and np.array_equal(np.where(D > 0, win, -1), np.where(Do > 0, wo, -1)), f
        for m, (pix, dep, idx) in enumerate(c.maps[f]):
            assert (c.inputs["masks"][f, m].ravel()[pix] > 0).all() and (dep > 0).all() and np.array_equal(win.ravel()[pix], idx)
            assert len(pix) == ((c.inputs["masks"][f, m] > 0) & (D > 0)).sum()
    assert (c.ref["car_len"] > 0).sum() >= 20 and (c.ref["car_len"][5] > 0).sum() == 2
    o = C.depth_overlays()
    for it in range(o.items):
        f, m = divmod(it, C.MD)
        pix = c.maps[f][m][0]
        rest = np.ones(cam["W"] * cam["H"], bool)
        rest[pix] = False
        assert np.array_equal(o.ref["images"][it].reshape(-1, 3)[rest], o.inputs["seg"][f][..., ::-1].reshape(-1, 3)[rest])
        assert o.ref["max_depth"][it] == (c.maps[f][m][1].max() if len(pix) else 0.0)


# ---- (b) neighbours differ -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", C.CALLS)
def test_adjacent_nonempty_items_have_different_outputs(call):
    c = C.case(call)
    items = np.flatnonzero(c.nonempty)
    assert len(items) >= 8
    sig = lambda i: b"|".join(np.ascontiguousarray(c.rows(k, i)).tobytes() for k in c.ref)
    for a, b in zip(items, items[1:]):
        assert sig(a) != sig(b), (call, a, b)
    for k in c.item_kind:                                    # and every per-item output tells some neighbours apart
        assert any(c.rows(k, a).tobytes() != c.rows(k, b).tobytes() for a, b in zip(items, items[1:])), (call, k)


# ---- (c) teeth -----------------------------------------------------------------------------------------------------------------------------
def _only_nothing_rows(c, cut, kind):
    """the forgery moves rows that hold the fill onto rows that hold the fill: the wrong base writes what the right one would"""
    for k in (c.item_kind if kind == "item" else c.frame_kind):
        s = c.spans[k]
        n = int(s[-1] - s[cut])
        fill = np.full(1, c.fill[k], c.ref[k].dtype)
        if (c.ref[k][int(s[cut]):] != fill).any() or (c.ref[k][:n] != fill).any():
            return False
    return True


@pytest.mark.parametrize("call", C.CALLS)
def test_compare_rejects_the_answer_of_a_wrong_base(call):
    c = C.case(call)
    assert C.compare(c.ref, c.ref) is None
    seen = {"item": 0, "frame": 0}
    for cut in range(1, c.items):
        for kind in ("item", "frame"):
            for clear in (False, True):
                forged = C.forge(c, cut, kind, clear)
                if forged is None or _only_nothing_rows(c, cut, kind):
                    continue
                assert C.compare(forged, c.ref) is not None, (call, cut, kind, clear)
                seen[kind] += 1
    assert seen["item"] >= c.items
    if call == "match_2d":
        assert not c.frame_kind                              # every output is per detection or per pair
    elif call == "assign_2d":
        # scores of finite weights always solve: status 0 in every frame, so the values alone cannot show a wrong status pointer.
        # The GPU sweep's "hhr" / "ddr" runs therefore hand the call a status array filled with a sentinel: a range whose memset
        # starts at range 1's base leaves the sentinel in its own rows, and compare() sees that
        assert not c.ref["status"].any() and seen["frame"] == 0
        for cut in range(1, c.items):
            assert C.compare(C.forge(c, cut, "frame", clear=True, fill=dict(c.fill, status=-7)), c.ref) is not None, cut
    else:
        assert seen["frame"] >= c.items // 2
