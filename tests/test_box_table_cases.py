"""What tests/box_table_cases.py claims, checked without a GPU: every finite laid-out point is valid under the cases' camera and lies in
mask 0; the Fraction yardstick agrees with the reference's NumPy statement and with the C oracle on every exact shape (both values of
``oriented``) and the oracle with Fraction on the generic class; the cases reach what they are there for (both sides of every face,
inside points beyond the corner AABB, both sides of the conditioning gate, all three 64-box words); the two wrong prefilter models
change counts in the sheared scenes; and the checker raises on one corrupted count.

One claim of the issue behind these cases does not hold and is pinned as it is: a prefilter without the |v_a|^2 factor (e_a = w_a) is
NOT invisible to orthogonal boxes in general -- it shrinks the bound of every cuboid with edges longer than a metre -- so it changes
nothing only in the scene of unit cubes; the corner-AABB prefilter changes nothing in any cuboid-only scene."""
import numpy as np
import pytest

import box_table_cases as C
from oracle import cpu_oracle as orc
from oracle import numpy_path as npp

SCENES = C.scenes()
NAMES = list(SCENES)
SCENE = pytest.mark.parametrize("name", NAMES)


def _numpy_inside(points, corners):
    with np.errstate(all="ignore"):
        return np.asarray(npp.oriented_point_in_bbox(points[:, :3], corners), bool)


@SCENE
def test_every_finite_point_is_valid_and_in_mask_0(name):
    s = SCENES[name]
    u, v, ok = s.pixels()
    fin = np.all(np.isfinite(s.points[:, :3]), axis=1)
    assert np.array_equal(ok, fin), (name, s.points[ok != fin][:4])
    assert np.count_nonzero(~fin) == 3
    assert np.all((u[ok] >= 21) & (u[ok] <= 43) & (v[ok] >= 11) & (v[ok] <= 21)), name
    for M in (3, 9, C.M_WIDE):
        mem = s.member(M)
        assert np.array_equal(mem[0], ok), (name, M)
        assert np.array_equal(mem[M - 1] if M == C.M_WIDE else mem[0], ok)
        assert not mem[:, ~ok].any()
    # the C oracle projects the same pixels
    o = orc.project(s.points, C.T, C.K)
    assert np.array_equal(o["u32"][ok], u[ok]) and np.array_equal(o["v32"][ok], v[ok]), name


def test_generic_points_are_valid():
    for fr in C.generic():
        o = orc.run(fr["points"], C.T, C.K, C.W, C.H, C.DMIN, C.DMAX, want_float=False)
        assert o["n_valid"] == len(fr["points"]) == C.GENERIC_POINTS * C.GENERIC_BOXES // C.GENERIC_FRAMES
        assert np.all(np.abs(fr["points"]) <= C.LIMIT)


@SCENE
def test_yardstick_agrees_with_numpy_statement_and_oracle(name):
    s = SCENES[name]
    for b, sh in enumerate(s.boxes):
        want = s.inside(True)[b]
        got = orc.points_in_box(s.points, sh.corners, oriented=True)
        assert np.array_equal(got, want), ("oracle", C.describe(s, b, int(np.flatnonzero(got != want)[0])))
        if sh.exact:
            got = _numpy_inside(s.points, sh.corners)
            assert np.array_equal(got, want), ("numpy", C.describe(s, b, int(np.flatnonzero(got != want)[0])))
        want = s.inside(False)[b]
        got = orc.points_in_box(s.points, sh.corners, oriented=False)
        assert np.array_equal(got, want), ("oracle, axis-aligned", C.describe(s, b, int(np.flatnonzero(got != want)[0])))


def test_integer_path_is_the_fraction_yardstick():
    """inside_matrix evaluates on-grid pairs in int64: the same as inside_fraction on every box's own points and on a seeded sample of
    the other pairs; and the double evaluation of every exact shape's own pairs is exact, operand by operand"""
    rng = np.random.default_rng(5)
    for s in SCENES.values():
        for oriented in (True, False):
            ins = s.inside(oriented)
            pairs = [(b, i) for i, b in enumerate(s.owner) if b >= 0 and s.boxes[b].exact]
            B = len(s.boxes)
            if B:
                pairs += [(int(b), int(i)) for b, i in zip(rng.integers(0, B, 300), rng.integers(0, len(s.points), 300)) if s.boxes[b].exact]
            for b, i in pairs:
                assert ins[b, i] == C.inside_fraction(s.points[i], s.corners[b], oriented), C.describe(s, b, i)
    for sh in C.shapes().values():
        if sh.exact:
            for p in sh.points:
                assert C.exact_in_double(p, sh.corners), (sh.name, p)


def test_replaced_corners():
    """corners 2, 5, 6, 7 moved to 2^22 or made NaN: the oriented result is the untouched cuboid's; the axis-aligned one takes the far
    corners in and skips the NaN ones (corner 0 is finite), as orc_aabb_inside states it"""
    sh = C.shapes()
    for name, c0 in (("replaced_far", (-6, -30, 1)), ("replaced_nan", (4, -30, 1))):
        s = sh[name]
        whole = C.corners_of(c0, *C.CUBOID)
        pts = np.concatenate([t.points for t in sh.values()])
        assert np.array_equal(C.inside_matrix(s.corners[None], pts), C.inside_matrix(whole[None], pts)), name
        a = C.inside_matrix(s.corners[None], pts, oriented=False)[0]
        if name == "replaced_far":
            assert a[np.all(pts == 1000, axis=1)].all() and a.sum() > C.inside_matrix(whole[None], pts, oriented=False).sum()
        else:
            c = whole[[0, 1, 3, 4]]
            want = np.all((pts >= c.min(0)) & (pts <= c.max(0)), axis=1)
            assert np.array_equal(a, want) and a.any()


def test_generic_class_oracle_agrees_with_fraction():
    """every box's own 64 points (none nearer than 2^-30 to a face, relative to the slab: nothing is excluded here) and a seeded sample
    of the other pairs of its frame"""
    rng = np.random.default_rng(6)
    n = 0
    for fr in C.generic():
        ins = C.generic_inside(fr)
        B, N = ins.shape
        for i, b in enumerate(fr["owner"]):
            assert C.slab_margins(fr["points"][i], fr["corners"][b]) >= C.MARGIN
            assert ins[b, i] == C.inside_fraction(fr["points"][i], fr["corners"][b]), (b, i)
        for b, i in zip(rng.integers(0, B, 5000), rng.integers(0, N, 5000)):
            assert ins[b, i] == C.inside_fraction(fr["points"][i], fr["corners"][b]), (b, i)
        own = ins[fr["owner"], np.arange(N)]
        assert 0.2 < own.mean() < 0.8                                    # the points are drawn around the region: both sides
        n += int(sum(C.float_bounds(c) is None for c in fr["corners"]))
        cond = [np.linalg.cond(np.array([(c[o] - c[0]) / np.linalg.norm(c[o] - c[0]) for o in C.OTHER])) for c in fr["corners"]]
        assert max(cond) <= 1e5 * (1 + 1e-9) and max(cond) > 1e3
    assert n > 0                                                         # some fall below the conditioning gate


# ---- what the cases reach ---------------------------------------------------------------------------------------------------------------------------
def _slabs(p, corners):
    c0, v, vv = C._edges(corners)
    r = [C._fr(p[i]) - c0[i] for i in range(3)]
    return [(sum(a * b for a, b in zip(r, va)), w) for va, w in zip(v, vv)]


def test_both_sides_of_every_face():
    for sh in C.shapes().values():
        ins = C.inside_matrix(sh.corners[None], sh.points, generic=() if sh.exact else (0,))[0]
        assert ins.any() and not ins.all(), sh.name
        if "vertex" not in sh.tags:
            continue
        for a in range(3):
            for side in "-+":
                out = [i for i, t in enumerate(sh.tags) if t == "out:%d%s" % (a, side)]
                assert out, (sh.name, a, side)
                for i in out:                                            # outside through this face alone
                    sl = _slabs(sh.points[i], sh.corners)
                    assert not ins[i]
                    assert all((0 <= d <= w) == (k != a) for k, (d, w) in enumerate(sl)), (sh.name, a, side)
                    assert (sl[a][0] < 0) == (side == "-")
                on = [i for i, t in enumerate(sh.tags) if t in ("vertex", "edge", "face") and ins[i]
                      and _slabs(sh.points[i], sh.corners)[a][0] == (0 if side == "-" else _slabs(sh.points[i], sh.corners)[a][1])]
                assert on or (sh.kind == "tiny" and side == "+"), (sh.name, a, side)      # inclusive: a point ON the face is inside
        if sh.kind != "tiny":
            assert sum(t in ("vertex", "edge", "face", "centre") for t in sh.tags) == 27 and \
                all(ins[i] for i, t in enumerate(sh.tags) if t in ("vertex", "edge", "face", "centre")), sh.name
    tiny = C.shapes()["tiny"]
    assert C.inside_matrix(tiny.corners[None], np.concatenate([s.points for s in C.shapes().values()]))[0].sum() == 1


def test_sheared_shapes_reach_beyond_the_corner_aabb():
    for name in C.SHEARED:
        sh = C.shapes()[name]
        ins = C.inside_matrix(sh.corners[None], sh.points)[0]
        c = sh.corners
        hull = np.array([c[0] + a * (c[1] - c[0]) + b * (c[3] - c[0]) + d * (c[4] - c[0]) for a in (0, 1) for b in (0, 1) for d in (0, 1)])
        in_aabb = np.all((sh.points >= hull.min(0)) & (sh.points <= hull.max(0)), axis=1)
        assert np.count_nonzero(ins & ~in_aabb) >= 1, name
        assert np.count_nonzero(~ins & in_aabb) >= 1, name
        assert all(ins[i] and not in_aabb[i] for i, t in enumerate(sh.tags) if t == "beyond_aabb")
        assert all(in_aabb[i] and not ins[i] for i, t in enumerate(sh.tags) if t == "aabb_not_region")
    # the issue's example: c0 = (8,-4,1), v = (4,0,0), (2,3,0), (1,1,2)
    c0, e = C.region_basis(C.corners_of((8, -4, 1), (4, 0, 0), (2, 3, 0), (1, 1, 2)))
    lo = [float(c0[i] + sum(min(e[a][i], 0) for a in range(3))) for i in range(3)]
    hi = [float(c0[i] + sum(max(e[a][i], 0) for a in range(3))) for i in range(3)]
    assert np.allclose(lo, [8, -4 - 8 / 3, 1 - 17 / 6]) and np.allclose(hi, [12, 1 / 3, 4])


def test_gate_shapes_fall_on_the_stated_sides():
    sh = C.shapes()
    for k, bounded in ((18, True), (19, True), (20, False), (21, False)):
        s = sh["gate_2^-%d" % k]
        d2, g = C.gate_sides(s.corners)
        assert (d2 > g) == bounded, (k, d2, g)
        assert (C.float_bounds(s.corners) is not None) == bounded
        ins = C.inside_matrix(s.corners[None], s.points)[0]
        assert np.any(ins & (np.abs(s.points[:, 2]) >= 2.0 ** 19)), k     # inside points far along the long edge
    for name in ("prism", "vv_huge", "vv_tiny", "gate_2^-20", "gate_2^-21"):
        assert C.float_bounds(sh[name].corners) is None, name
    p = sh["prism"]
    ins = C.inside_matrix(p.corners[None], p.points)[0]
    assert np.any(ins & (p.points[:, 2] == 2.0 ** 20)) and np.any(ins & (p.points[:, 2] == -2.0 ** 20))      # the infinite prism
    for name in ("overflow", "overflow_negative"):
        lo, hi = C.float_bounds(sh[name].corners)
        assert np.isinf(hi).all() if name == "overflow" else np.isinf(lo).all(), name
    for name, lim in (("plate", 2.0 ** -20), ("needle", 2.0 ** -20)):
        c = sh[name].corners
        n = sorted(np.linalg.norm(c[o] - c[0]) for o in C.OTHER)
        assert n[0] / n[2] == lim, name


def test_scenes_put_the_special_boxes_into_the_stated_words():
    assert sorted({len(s.boxes) for s in SCENES.values()}) == [0, 1, 5, 63, 64, 65, 129]
    for s in SCENES.values():
        B = len(s.boxes)
        assert len(s.points) <= 20000
        for b, n in s.special.items():
            assert s.boxes[b].name == n
        if s.kind == "sheared" and B > 5:
            for b in (0, 63, 64, B - 1):
                if b < B:
                    assert b in s.special, (s.name, b)
            assert {C.word_of(b) for b in s.special} == set(range((B + 63) // 64)), s.name
    assert {C.word_of(b) for b, n in SCENES["b129"].special.items() if n in C.SHEARED} == {0, 1, 2}
    assert C.masks_of("b129") * 129 > 1024
    assert [len(SCENES[n].boxes) for n in C.BATCH3] == [129, 0, 5]
    # the far box stretches its word's domain: the near boxes share one cell of 32
    s = SCENES["b64"]
    x0, y0, x1, y1 = s.domain(0)
    assert "far" in s.special.values() and (x1 - x0) / 32 > 1e5
    near = [C.float_bounds(c) for b, c in enumerate(s.corners) if s.boxes[b].name != "far" and C.float_bounds(c) is not None]
    assert len(near) >= 61 and all(int((hi[0] - x0) / (x1 - x0) * 32) == 0 for _, hi in near)
    # a word of unbounded boxes only has no domain
    s = SCENES["b129_unbounded_word"]
    assert s.domain(1) is None and s.domain(0) is not None and s.domain(2) is not None
    assert s.inside()[64:128].sum() > 64
    for s in SCENES.values():                                            # grid-border points and points outside the domain, per word
        for w in range((len(s.boxes) + 63) // 64):
            d = s.domain(w)
            p = s.points[[t == "border:%d" % w for t in s.tags]]
            assert len(p) >= 16
            if d is not None and max(abs(float(x)) for x in d) + 8 <= C.LIMIT:
                assert {d[0], d[2]} <= set(p[:, 0]) and {d[1], d[3]} <= set(p[:, 1])
                assert (p[:, 0] < d[0]).any() and (p[:, 0] > d[2]).any() and (p[:, 1] < d[1]).any() and (p[:, 1] > d[3]).any()


# ---- the wrong models -----------------------------------------------------------------------------------------------------------------------------------
def test_stated_bounds_lose_nothing():
    """the float bounds as the box job states them are a superset of the accepted region in every scene, for both tests"""
    for s in SCENES.values():
        M = C.masks_of(s.name)
        for oriented in (True, False):
            assert np.array_equal(C.model_counts(s, "stated", M, oriented), s.expected(M, oriented)["count_mb"]), (s.name, oriented)
    for fr in C.generic():
        ins = C.generic_inside(fr)
        for b, c in enumerate(fr["corners"]):
            fb = C.float_bounds(c)
            if fb is not None:
                p = fr["points"][ins[b], :3]
                assert np.all((p >= fb[0]) & (p <= fb[1])), b


def test_wrong_models_are_caught_by_the_sheared_scenes_only():
    caught = {m: [] for m in C.MODELS[1:]}
    for s in SCENES.values():
        M = C.masks_of(s.name)
        want = s.expected(M)["count_mb"]
        for m in C.MODELS[1:]:
            got = C.model_counts(s, m, M)
            assert np.all(got <= want)
            if not np.array_equal(got, want):
                caught[m].append(s.name)
                if s.kind == "sheared":                                  # and the checker says so
                    with pytest.raises(AssertionError, match="outside the stated float bounds|count"):
                        C.check_counts(s, m, dict(count_mb=got), M, keys=("count_mb",))
    sheared = {n for n, s in SCENES.items() if s.kind == "sheared"}
    for m in C.MODELS[1:]:
        assert sheared <= set(caught[m]), (m, caught[m])                 # every scene with a sheared shape sees either model
    assert set(caught["prefilter_by_corner_aabb"]) <= sheared            # no cuboid-only scene sees it
    assert "one" in caught["prefilter_by_corner_aabb"]
    # e_a = w_a: invisible to the unit cubes only -- any cuboid with an edge above a metre already falls out of that bound
    assert "unit_cuboids" not in caught["prefilter_without_vv"] and "cuboids" in caught["prefilter_without_vv"]


def test_checker_raises_on_one_corrupted_count():
    s = SCENES["b129"]
    M = C.masks_of("b129")
    want = s.expected(M)
    C.check_counts(s, "self", want, M)
    bad = dict(want, count_mb=want["count_mb"].copy())
    b = 64
    assert bad["count_mb"][0, b] > 0
    bad["count_mb"][0, b] -= 1
    with pytest.raises(AssertionError) as e:
        C.check_counts(s, "corrupted", bad, M)
    msg = str(e.value)
    assert "corrupted" in msg and "b129" in msg and "box 64" in msg and "word 1" in msg and s.boxes[b].name in msg and "point" in msg
    bad = dict(want, best_box=want["best_box"].copy())
    bad["best_box"][1] += 1
    with pytest.raises(AssertionError, match="best_box"):
        C.check_counts(s, "corrupted", bad, M)
    ins = np.array(s.inside())
    ins[128, np.flatnonzero(ins[128])[0]] = False
    with pytest.raises(AssertionError, match="box 128.*word 2"):
        C.check_inside(s, "corrupted", ins)


def test_pair_census():
    """what the GPU test covers per path (the numbers the summary of the change quotes)"""
    tot = {}
    for s in SCENES.values():
        for k, v in C.pair_census(s).items():
            tot[k] = tot.get(k, 0) + v
    print("pairs per pass over the scenes:", tot)
    assert tot["beyond_corner_aabb"] > 0 and tot["on_face"] > 0 and tot["in_unbounded_box"] > 0 and tot["inside_beyond_first_word"] > 0
