"""The CPU side of the edge-value projection cases (tests/projection_cases.py): the C oracle against the exact restatement and against
the NumPy statements of the reference, tests/box_views_ref.py against both on the cam-0 corner sets, and what the cases reach.  The
GPU side is tests/test_gpu_projection_edges.py: it compares every route with the oracle, so the oracle's own edge conventions are
pinned here, outside its source."""
import numpy as np
import pytest

import box_views_ref as bv
import projection_cases as P
from conftest import load_calib
from oracle import cpu_oracle as orc
from oracle import numpy_path as npp

CALIB = load_calib()
CAMS = P.cameras(CALIB)
NAMES = [c["name"] for c in CAMS]
FLOATS = ("uf", "vf", "depth")


def _exact_pixels(x):
    u = np.array([P.sat_i32(P.rint(a)) for a in x["uf"]], np.int64)
    v = np.array([P.sat_i32(P.rint(a)) for a in x["vf"]], np.int64)
    return u, v


def _exact_valid(cam, x):
    return np.array([P.is_valid(a, b, d, cam["W"], cam["H"], cam["dmin"], cam["dmax"]) for a, b, d in zip(x["uf"], x["vf"], x["depth"])], bool)


@pytest.mark.parametrize("index", range(len(CAMS)), ids=NAMES)
def test_oracle_equals_the_exact_projection(index):
    """orc.project and orc.run on every point of the camera's cloud: uf, vf and depth as bit patterns (the sign of a zero included,
    NaN by position), the saturated pixels, the valid set and the full mask's list"""
    cam = CAMS[index]
    pts = P.cloud(CALIB, index)
    x = P.exact_cloud(pts, cam["T"], cam["K"])
    u, v = _exact_pixels(x)
    valid = _exact_valid(cam, x)
    o = orc.project(pts, cam["T"], cam["K"])
    for k in FLOATS:
        assert P.same_floats(o[k], x[k]), (cam["name"], "project", k)
    assert np.array_equal(o["u32"], u) and np.array_equal(o["v32"], v), cam["name"]
    lab = orc.pack_masks(P.masks(cam), 0, cam["H"], cam["W"])
    r = orc.run(pts, cam["T"], cam["K"], cam["W"], cam["H"], cam["dmin"], cam["dmax"], label_img=lab, M=3, corners=P.boxes(cam, pts))
    for k in FLOATS:
        assert P.same_floats(r[k], x[k]), (cam["name"], "run", k)
    assert np.array_equal(r["u"], u) and np.array_equal(r["v"], v), cam["name"]
    assert np.array_equal(r["valid_idx"], np.flatnonzero(valid)) and r["n_valid"] == int(valid.sum()), cam["name"]
    assert np.array_equal(r["inst_lists"][0], np.flatnonzero(valid)), cam["name"]                # the full mask lists every valid point
    right = valid & (np.array([P.rint(a) for a in x["uf"]]) >= cam["W"] // 2)
    assert np.array_equal(r["inst_lists"][1], np.flatnonzero(right)) and r["inst_count"][2] == 0, cam["name"]
    D, win = orc.depth_image(pts, cam["T"], cam["K"], cam["W"], cam["H"], cam["dmin"], cam["dmax"])
    want_win = np.full(cam["W"] * cam["H"], -1, np.int64)
    vi = np.flatnonzero(valid)
    want_win[v[vi] * cam["W"] + u[vi]] = vi                                                      # ascending: the last valid point wins
    assert np.array_equal(win.ravel(), want_win), cam["name"]
    assert P.same_floats(D.ravel(), np.where(want_win >= 0, x["depth"][np.maximum(want_win, 0)], 0.0)), cam["name"]


@pytest.mark.parametrize("index", range(len(CAMS)), ids=NAMES)
def test_oracle_equals_the_numpy_statements(index):
    """orc.project against cam2image behind np.matmul(T, points_homo.T), as oracle/numpy_path.frame_path writes them: depth bit for
    bit, u and v wherever the rounded value is below 2^63 in magnitude.  Beyond that (and for NaN) ``astype(int)`` is
    platform-defined -- NumPy on x86-64 gives INT64_MIN where the ABI saturates to INT32_MAX -- and the ABI's own convention in
    include/lpf.h (saturate, NaN -> INT32_MIN) is the specification, held by test_oracle_equals_the_exact_projection.  No such pixel
    is ever valid."""
    cam = CAMS[index]
    pts = np.array(P.cloud(CALIB, index))
    homo = pts.copy()
    homo[:, 3] = 1
    with np.errstate(invalid="ignore", over="ignore"):
        cam_pts = np.matmul(cam["T"], homo.T).T[:, :3]
        u, v, depth = npp.cam2image(cam["K"], cam_pts.T)
    o = orc.project(pts, cam["T"], cam["K"])
    assert P.same_floats(o["depth"], depth), cam["name"]
    for got64, got32, want, f in ((o["u64"], o["u32"], u, o["uf"]), (o["v64"], o["v32"], v, o["vf"])):
        with np.errstate(invalid="ignore"):
            defined = np.abs(np.rint(f)) < 2.0 ** 63                                           # (False for NaN)
        assert np.array_equal(got64[defined], want[defined]), cam["name"]
        assert np.array_equal(got32[defined], np.clip(want[defined], P.I32_MIN, P.I32_MAX)), cam["name"]
        valid = np.zeros(len(pts), bool)
        valid[orc.run(pts, cam["T"], cam["K"], cam["W"], cam["H"], cam["dmin"], cam["dmax"], want_float=False)["valid_idx"]] = True
        assert not (valid & ~defined).any(), cam["name"]


@pytest.mark.parametrize("e", P.BOX_SCALES)
def test_box_views_ref_equals_the_exact_projection_and_the_numpy_statements(e):
    """tests/box_views_ref.py (the restatement the GPU's box routes are held against) on the cam-0 corner sets: front and bbox2d
    against exact_project, visible against exact_project and against numpy_path.prepare_boxes, corners_velo against prepare_boxes"""
    corners, names = P.box_corner_sets()
    K, W, H = P.box_K(e), P.BOX_W, P.BOX_H
    Tvc = np.asarray(CALIB["TrVeloToCam"], np.float64)
    visible, front, bbox2d, ru, rv, d = P.exact_boxes(corners, K, W, H)
    ref = bv.views(corners, [0, len(corners)], K, W, H, np.linalg.inv(Tvc), want=("front", "bbox2d", "corners_velo"))
    assert np.array_equal(ref["front"], front), [n for n, a, b in zip(names, ref["front"], front) if a != b]
    assert P.same_floats(ref["bbox2d"], bbox2d), [n for n, a, b in zip(names, ref["bbox2d"], bbox2d) if not P.same_floats(a, b)]
    u, v, dd = bv.project(corners, K)
    assert P.same_floats(u, ru) and P.same_floats(v, rv) and P.same_floats(dd, d)
    vis_np, velo_np = npp.prepare_boxes(corners, K, W, H, Tvc)
    assert np.array_equal(vis_np, visible), [n for n, a, b in zip(names, vis_np, visible) if a != b]
    assert bv.same_bits(ref["corners_velo"], velo_np)
    # the reference's own pixels are integers (cam2image's astype(int)), which have one zero: number for number, its boxes are these
    checked = 0
    for b in range(len(corners)):
        fr = d[b] > 0
        if fr.any() and (np.abs(ru[b][fr]) < 2.0 ** 63).all() and (np.abs(rv[b][fr]) < 2.0 ** 63).all():
            ui, vi, _ = npp.cam2image(K, corners[b].T.copy())
            assert np.array_equal(ref["bbox2d"][b], [ui[fr].min(), vi[fr].min(), ui[fr].max(), vi[fr].max()]), names[b]
            checked += 1
    assert checked >= 10


def test_what_the_point_cases_reach():
    """Conditions on the generator: every class of projection_cases.CLASSES is reached by some camera, the window classes by the
    cameras built for them, and every camera with a non-empty window has valid points -- in the full cloud and in E alone."""
    E = P.edge_points()
    pos = P.edge_positions()
    for edge in P.STRADDLE:                                   # a copy of E lies across 63|64, 1023|1024 and 4095|4096
        assert any(a < edge < a + len(E) for a in pos), (edge, pos)
    table = {}
    for index, cam in enumerate(CAMS):
        full = P.cloud(CALIB, index)
        assert len(full) <= 6000 and pos[0] == 0 and pos[-1] + len(E) == len(full)
        for a in pos:
            assert full[a:a + len(E)].tobytes() == E.tobytes()
        c = table[cam["name"]] = P.classes(cam, full)
        if cam["dmax"] > cam["dmin"]:
            assert c["valid"] > 0 and P.classes(cam, E)["valid"] > 0, cam["name"]
        else:
            assert c["valid"] == 0, cam["name"]
        assert c["nan"] > 0, cam["name"]
    for k in P.CLASSES:
        assert any(c[k] for c in table.values()), k
    t = lambda name: table[name]
    for name in NAMES:
        if name.startswith("ties_") or name.startswith("scaled_"):
            assert t(name)["sat_i32"] > 0 and (t(name)["valid"] == 0 or (t(name)["tie_even"] > 0 and t(name)["tie_odd"] > 0)), name
    assert t("ties_0_50")["d0_invalid"] > 0 and t("ties_0_50")["on_dmax"] > 0
    assert t("ties_0.5_30")["on_dmin"] > 0 and t("ties_0.5_30")["on_dmax"] > 0
    for name in ("ties_m5_50", "ties_minf_inf"):
        assert t(name)["d0_valid"] > 0 and t(name)["d0_invalid"] > 0 and t(name)["behind_valid"] > 0, name
    assert t("ties_m5_50")["on_dmin"] > 0
    # the scaled cameras: the same pixels and the same valid set as the ties camera of the window (0, 50)
    base = P.exact_cloud(P.cloud(CALIB, NAMES.index("ties_0_50")), CAMS[0]["T"], CAMS[0]["K"])
    for index, cam in enumerate(CAMS):
        if cam["kind"] == "scaled":
            x = P.exact_cloud(P.cloud(CALIB, index), cam["T"], cam["K"])
            d0 = base["depth"] == -1e-6                       # (the substitute depth is not scaled: those points are invalid in both)
            assert P.same_floats(x["uf"][~d0], base["uf"][~d0]) and P.same_floats(x["vf"][~d0], base["vf"][~d0]), cam["name"]
            assert t(cam["name"])["valid"] == t("ties_0_50")["valid"], cam["name"]
    assert t("scaled_m302")["qx_below"] and t("scaled_m302")["qy_below"] and t("scaled_m302")["d_below"]       # across 722 | 723 ...
    assert t("scaled_296")["qx_above"] and t("scaled_296")["qy_above"]                                           # ... and 1323 | 1324
    inside = [k for k in P.CLASSES if k.endswith("_below") or k.endswith("_above")]
    assert not any(t("scaled_40")[k] for k in inside)
    alone = dict(zip(("qx_below", "qx_above", "qy_below", "qy_above", "d_below", "d_above"), [n for n in NAMES if n.startswith("diag_")]))
    for k, name in alone.items():                             # each operand alone outside the window, each side, and inside it too
        assert t(name)[k] > 0 and not any(t(name)[j] for j in inside if j != k), (name, k)
        x = P.exact_cloud(P.cloud(CALIB, NAMES.index(name)), np.eye(4), CAMS[NAMES.index(name)]["K"])
        op = np.abs(x["depth"]) if k.startswith("d_") else x["qx"] if k.startswith("qx") else x["qy"]
        e = P.biased_exponent(op)
        assert ((e >= P.DIV2_LO) & (e <= P.DIV2_HI)).any(), (name, k)
        assert (e == (P.DIV2_LO - 1 if k.endswith("below") else P.DIV2_HI + 1)).any(), (name, k)      # the binade next to the window
        assert (e == (P.DIV2_LO if k.endswith("below") else P.DIV2_HI)).any(), (name, k)              # and its first one inside
    assert t("diag_600_600_m600")["quot_inf"] > 0
    assert t("diag_m530_m530_520")["quot_subnormal"] > 0
    assert t("diag_m600_m600_600")["quot_zero"] > 0
    print("\n" + "\n".join("%-22s %s" % (n, " ".join("%s=%d" % (k, v) for k, v in table[n].items() if v)) for n in NAMES))


def test_what_the_corner_sets_reach():
    """Conditions on the corner sets, from exact_project and Fraction alone: every operand on each side of lpf_div2's window alone,
    under K = I and under both scaled K's; zero and subnormal numerators; a substituted depth; d on 0.1 and on its two neighbours,
    deciding visibility; exact ties at 0, W and H; near ties that land on each side; 0, 1, 2 and 8 corners in front."""
    from fractions import Fraction
    corners, names = P.box_corner_sets()
    flat = corners.reshape(-1, 3)
    expo = P.biased_exponent(np.abs(flat))
    inside = (expo >= P.DIV2_LO) & (expo <= P.DIV2_HI)
    for k in range(3):
        others = inside[:, [j for j in range(3) if j != k]].all(axis=1)
        assert (others & (expo[:, k] == P.DIV2_LO - 1)).any() and (others & (expo[:, k] == P.DIV2_LO)).any(), k
        assert (others & (expo[:, k] == P.DIV2_HI + 1)).any() and (others & (expo[:, k] == P.DIV2_HI)).any(), k
    for e in P.BOX_SCALES[1:]:                                # the scaled K's move ordinary corners across the window's edges
        scaled = P.biased_exponent(np.abs(flat) * 2.0 ** e)
        assert ((scaled >= 1) & (scaled < P.DIV2_LO)).any() if e < 0 else ((scaled > P.DIV2_HI) & (scaled < 2047)).any()
    assert (flat[:, 0] == 0).any() and (P.biased_exponent(flat[:, 0])[flat[:, 0] != 0] == 0).any()
    visible, front, bbox2d, ru, rv, d = P.exact_boxes(corners, P.box_K(0), P.BOX_W, P.BOX_H)
    assert (d == -1e-6).any() and ((d > 0) & (d < 1e-300)).any() and ((d < 0) & (d > -1e-300)).any()
    by = dict(zip(names, range(len(names))))
    assert not visible[by["z_0.1"]] and not visible[by["z_0.1_down"]] and visible[by["z_0.1_up"]]
    assert [int(front[by["front_%d" % k]]) for k in (0, 1, 2, 8)] == [0, 1, 2, 8]
    assert np.array_equal(bbox2d[by["front_0"]], [P.BIG, P.BIG, -P.BIG, -P.BIG])
    assert sorted(ru[by["u_ties"]].tolist()) == [-2.0, -0.0, 0.0, 2.0, 2.0, 14.0, 16.0, 16.0] and np.signbit(ru[by["u_ties"]][0])
    assert sorted(rv[by["v_ties"]].tolist()) == [-2.0, -0.0, 0.0, 2.0, 2.0, 6.0, 8.0, 8.0]
    below = above = 0
    for n, z in P.NEAR_TIES:
        b = by["near_tie_%d_%g" % (n, z)]
        for col, r in ((0, ru), (1, rv)):
            k0 = 3 * col
            tie = Fraction(corners[b, k0, col]) / Fraction(z)
            assert tie.denominator == 2
            for k, side in ((k0 + 1, -1), (k0 + 2, 1)):       # one ulp down, one ulp up: the exact quotient is no tie any more
                q = Fraction(corners[b, k, col]) / Fraction(z)
                assert (q < tie) if side < 0 else (q > tie)
                lands = r[b, k] - float(tie - Fraction(1, 2))     # 0: on n, 1: on n + 1 (r: rint of the correctly rounded quotient)
                assert lands in (0.0, 1.0), (n, z, col, side)
                below += side < 0 and lands == 0.0
                above += side > 0 and lands == 1.0
    assert below >= 5 and above >= 5
