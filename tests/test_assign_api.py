"""lpf_assign_costs / lpf_assign_2d without a GPU: the Python restatement of the solver (tests/assign_ref.py) against
scipy.optimize.linear_sum_assignment on the seeded case list and on small matrices, the golden file against both, the header and the
library's exports, the pipeline's shared reporting code with pairs assigned elsewhere, and the batched matchers' device route on a
context whose lpf_assign_2d is the restatements."""
import contextlib
import ctypes
import hashlib
import io
import os
import re

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import assign_ref as A
import match2d_ref as R
from conftest import GOLDEN
from lidar_object_detection_amd import _build, _native, pipeline
from test_match2d_api import _RefContext, _boxes_of, _golden, golden_frame

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case_list():
    return A.cases()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "assign_golden.npz"))


def _same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


def test_restatement_equals_scipy_on_the_case_list(case_list):
    assert len(case_list) == 12 * 5 + 2 and {m.shape for _, m in case_list} == set(A.SHAPES)
    for name, m in case_list:
        st, rows, cols = A.solve(m)
        assert st == A.OK and _same((rows, cols), linear_sum_assignment(m)), name
        assert rows.dtype == np.int64 and cols.dtype == np.int64


def test_restatement_equals_scipy_on_3000_small_matrices_with_both_forms_of_the_argmin():
    wrong_first = wrong_asc = n_int = 0
    for k, m in enumerate(A.small_cases(3000)):
        exp = linear_sum_assignment(m)
        assert _same(A.solve(m)[1:], exp), k
        assert _same(A.solve(m, argmin=A._argmin_scan)[1:], exp), k
        if k % 4 == 0 and k < 1600:                          # the tie-heavy integer kind: the two wrong solvers do disagree
            n_int += 1
            wrong_first += not _same(A.solve(m, first_min=True)[1:], exp)
            wrong_asc += not _same(A.solve(m, ascending=True)[1:], exp)
    assert n_int == 400 and wrong_first > 100 and wrong_asc > 100, (wrong_first, wrong_asc)


def test_status_and_front():
    m = np.array([[1.0, np.inf, 3.0], [np.inf, np.inf, 2.0]])
    st, rows, cols = A.solve(m)
    assert st == A.OK and _same((rows, cols), linear_sum_assignment(m))
    bad = np.array([[1.0, np.inf], [2.0, np.inf]])
    assert A.solve(bad)[0] == A.INFEASIBLE
    with pytest.raises(ValueError, match="cost matrix is infeasible"):
        linear_sum_assignment(bad)
    for v in (np.nan, -np.inf):
        x = np.ones((3, 4))
        x[1, 2] = v
        assert A.solve(x)[0] == A.INVALID
        with pytest.raises(ValueError, match="matrix contains invalid numeric entries"):
            linear_sum_assignment(x)
    assert A.solve(np.zeros((0, 4)))[0] == A.OK and A.solve(np.zeros((3, 0)))[0] == A.OK
    rng = np.random.default_rng(3)
    c = A.matrix(rng, "int012", 9, 14)
    front = (np.arange(14) % 3 != 1).astype(np.int32)
    st, rows, cols = A.solve_front(c, front)
    live = np.flatnonzero(front)
    er, ec = linear_sum_assignment(c[:, live])
    assert st == A.OK and np.array_equal(rows, er) and np.array_equal(cols, live[ec])
    x = c.copy()
    x[:, 1] = np.nan                                         # a dropped column's entries do not count
    assert A.solve_front(x, front)[0] == A.OK


def test_golden_case_list_is_the_seeded_one_with_scipys_answers(case_list, gold):
    assert gold["case_names"].tolist() == [n for n, _ in case_list]
    stored = 0
    for name, m in case_list:
        if "case_" + name in gold.files:
            assert np.array_equal(gold["case_" + name], m), name
            stored += 1
        else:
            assert str(gold["case_" + name + "_sha"]) == hashlib.sha256(np.ascontiguousarray(m).tobytes()).hexdigest(), name
        st, rows, cols = A.solve(m)
        assert np.array_equal(rows, gold["case_" + name + "_rows"]) and np.array_equal(cols, gold["case_" + name + "_cols"]), name
    assert stored >= 45


def test_golden_v5_runs(gold):
    frames, counts = gold["frames"].tolist(), gold["counts"].tolist()
    assert len(frames) == 19 and counts == [5, 32, 256]
    tall = wide = rejected = 0
    for f in frames:
        for n in counts:
            key = "%d_%d_" % (f, n)
            assert gold[key + "dets"].shape == (n, 4) and gold[key + "dets"].dtype == np.float32
            rows, cols = gold[key + "rows"], gold[key + "cols"]
            assert len(rows) == len(cols) and (np.diff(rows) > 0).all() and len(set(cols.tolist())) == len(cols)
            tall += len(rows) < n
            wide += len(rows) == n
            rejected += "Rejected match" in str(gold[key + "v5_stdout"])
            assert len(gold[key + "v5_box"]) == len(gold[key + "v5_colors"])
    assert tall >= 10 and wide >= 10 and rejected >= 10


def test_header_declares_the_entry_points_and_the_library_exports_them():
    text = open(os.path.join(REPO, "include", "lpf.h")).read()
    assert re.search(r"#define LPF_ABI_VERSION 8\b", text) and re.search(r"#define LPF_ASSIGN_MAX 1024\b", text)
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int lpf_assign_costs\(lpf_ctx \*ctx, int F, const lpf_assign_input \*in, const lpf_assign_outputs \*out\);", plain)
    assert re.search(r"int lpf_assign_2d\(lpf_ctx \*ctx, int F, const lpf_match2d_input \*in, const lpf_assign2d_params \*p, "
                     r"const lpf_assign2d_outputs \*out\);", plain)
    _build.build()
    lib = ctypes.CDLL(_native.library_path())
    assert hasattr(lib, "lpf_assign_costs") and hasattr(lib, "lpf_assign_2d")
    lib.lpf_abi_version.restype = ctypes.c_int
    assert lib.lpf_abi_version() == 8
    assert _native.LPF_ASSIGN_MAX == 1024 == A.CAP
    assert ctypes.sizeof(_native.AssignInput) == 40 and ctypes.sizeof(_native.AssignOutputs) == 24
    assert ctypes.sizeof(_native.Assign2dParams) == 16 and ctypes.sizeof(_native.Assign2dOutputs) == 64


def test_report_from_assigned_pairs_equals_the_report_from_matrices():
    """_improved_assign with the pairs a device call returns (detection, COMPACT column, scores, accepted) against the same function
    on the matrices: the lists and every printed line, the "Rejected match" line's compact column among them."""
    rng = np.random.default_rng(11)
    D, B = 9, 14
    valid = [j for j in range(B) if j % 4 != 2]
    m = {k: rng.random((D, len(valid))) for k in ("iou", "center", "size", "total")}
    m["cost"] = 1.0 - m["total"]
    boxes = [{"corners_velo": rng.random((8, 3)).tolist()} if j != 5 else {} for j in range(B)]
    colors = [(10 * i, 20, 30) for i in range(D - 2)]
    dets = np.zeros((D, 4), np.float32)
    rows, cols = linear_sum_assignment(m["cost"])
    pairs = [(int(i), int(j), float(m["iou"][i, j]), float(m["center"][i, j]), float(m["size"][i, j]), float(m["total"][i, j]),
              bool(m["total"][i, j] >= 0.3 and m["iou"][i, j] >= 0.15)) for i, j in zip(rows, cols)]
    a, b = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(a):
        host = pipeline._improved_assign(dets, boxes, colors, (valid, m))
    with contextlib.redirect_stdout(b):
        dev = pipeline._improved_assign(dets, boxes, colors, (valid, pairs))
    assert a.getvalue() == b.getvalue() and "Rejected match" in a.getvalue() and "Matched detection" in a.getvalue()
    assert len(host) == len(dev) > 0
    for (hc, hcol), (dc, dcol) in zip(host, dev):
        assert np.array_equal(hc, dc) and type(hcol) is type(dcol) and np.array_equal(np.asarray(hcol), np.asarray(dcol))
    with pytest.raises(ValueError, match="assign is"):
        pipeline.improved_match_detections_frames([], [], [], None, assign="gpu")


class _RefAssignContext(_RefContext):
    """_RefContext with lpf_assign_2d as well: the score restatement, the solver restatement on the cost, the two thresholds"""
    def __init__(self):
        super().__init__()
        self.assign_calls, self.match_frames = 0, []

    def match_2d(self, dets, bbox2d, front, **kw):
        self.match_frames.append([len(d) for d in dets])
        return super().match_2d(dets, bbox2d, front, **kw)

    def assign_2d(self, dets, bbox2d, front, weights=(0.5, 0.3, 0.2), min_score_threshold=0.3, min_iou_threshold=0.15,
                  want=_native.LpfContext.ASSIGN2D_WANT):
        self.assign_calls += 1
        _native.LpfContext.match2d_batch(dets, bbox2d, front)
        res = {k: [] for k in want if k != "status"}
        status = np.zeros(len(dets), np.int32)
        for f, (d, b, fr) in enumerate(zip(dets, bbox2d, front)):
            assert len(d) <= A.CAP and int((np.asarray(fr) > 0).sum()) <= A.CAP, "the library refuses this frame"
            m = R.score(d, b, fr, weights)
            status[f], rows, cols = A.solve_front(m["cost"], (np.asarray(fr) > 0).astype(np.int32))
            one = {"box_of_det": np.full(len(d), -1, np.int32), "accepted": np.zeros(len(d), np.int32)}
            one["box_of_det"][rows] = cols
            for k in ("iou", "center", "size", "total"):
                one[k] = np.zeros(len(d), np.float64)
                one[k][rows] = m[k][rows, cols]
            one["accepted"][rows] = (m["total"][rows, cols] >= min_score_threshold) & (m["iou"][rows, cols] >= min_iou_threshold)
            for k in res:
                res[k].append(one[k])
        if "status" in want:
            res["status"] = status
        return res


def _same_lists(got, exp):
    assert len(got) == len(exp)
    for (gc, gcol), (ec, ecol) in zip(got, exp):
        assert type(gc) is type(ec) and gc.dtype == ec.dtype and np.array_equal(gc, ec)
        assert type(gcol) is type(ecol) and np.array_equal(np.asarray(gcol), np.asarray(ecol))


def test_device_route_of_the_batched_matcher_equals_the_scalar_one_on_the_golden_frames():
    """improved_match_detections_frames with assign="device" and assign="host" against improved_match_detections_to_bboxes frame by
    frame, lists and printed lines: the 19 golden frames, a frame without detections, one without boxes, one with two boxes that were
    never transformed -- and then with a frame beyond LPF_ASSIGN_MAX detections among them, which alone takes the host route."""
    z = _golden()
    gs = [golden_frame(z, f) for f in z["frames"].tolist()]
    assert len(gs) == 19 and sum(bool((g["front"] <= 0).any()) for g in gs) >= 10       # a compact column is not the box's index
    dets = [g["dets"] for g in gs] + [np.zeros((0, 4), np.float32), gs[0]["dets"]]
    boxes = [_boxes_of(g, True) for g in gs] + [_boxes_of(gs[0], True), []]
    for j in (1, 4):
        del boxes[2][j]["corners_velo"]
    big_d, big_bb, big_front = R.cases(5, _native.LPF_ASSIGN_MAX + 1, 3, fraction=True)
    big_front[:] = 8
    dets_big = dets[:4] + [big_d] + dets[4:]
    boxes_big = boxes[:4] + [_boxes_of({"bbox2d": big_bb, "front": big_front}, True)] + boxes[4:]

    def scalar(dets, boxes, colors):
        out, buf = [], io.StringIO()
        with contextlib.redirect_stdout(buf):
            for d, b, c in zip(dets, boxes, colors):
                out.append(pipeline.improved_match_detections_to_bboxes(d, b, c, None))
        return out, buf.getvalue()

    def batched(dets, boxes, colors, assign):
        ctx, buf = _RefAssignContext(), io.StringIO()
        with contextlib.redirect_stdout(buf):
            out = pipeline.improved_match_detections_frames(dets, boxes, colors, None, ctx=ctx, assign=assign)
        return out, buf.getvalue(), ctx

    for ds, bs, big in ((dets, boxes, None), (dets_big, boxes_big, 4)):
        colors = [pipeline.generate_consistent_colors(max(len(d) - 1, 0)) for d in ds]      # one short: V5's red fallback
        exp, exp_text = scalar(ds, bs, colors)
        for line in ("Matched detection", "Rejected match", "No valid 3D bbox projections found", "Added unmatched"):
            assert line in exp_text, line
        got, text, ctx = batched(ds, bs, colors, "device")
        assert ctx.assign_calls == 1 and ctx.match_frames == ([] if big is None else [[_native.LPF_ASSIGN_MAX + 1]])
        for g, e in zip(got, exp):
            _same_lists(g, e)
        assert len(got) == len(exp) and text == exp_text
        got, text, ctx = batched(ds, bs, colors, "host")
        assert ctx.assign_calls == 0 and len(ctx.match_frames) == 1
        for g, e in zip(got, exp):
            _same_lists(g, e)
        assert len(got) == len(exp) and text == exp_text
