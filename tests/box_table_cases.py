"""Box shapes and laid-out points for the three structures the box job builds per frame (boxp, boxq and the ground grid cand: see
lpf_box_frame_block), with membership that is exact by construction.  Not a test module: tests/test_box_table_cases.py holds the
yardstick against the NumPy statement and the C oracle and asserts what the cases reach; tests/test_gpu_box_tables.py sends the scenes
through every consumer of the tables.

The yardstick is inside_fraction: the reference's oriented_point_in_bbox, 0 <= (p - c0) . v_a / |v_a|^2 <= 1 for v_a = c1 - c0,
c3 - c0, c4 - c0, evaluated in fractions.Fraction (oriented = 0: p between the minimum and the maximum of the 8 corners, a NaN corner
skipped unless it is corner 0, as orc_aabb_inside states it).  The exact shapes keep every product and sum of the double evaluation
exact (exact_in_double checks it operand by operand), so the reference's 0 <= d / vv <= 1 is 0 <= d <= vv in any summation order.
Their coordinates are dyadic -- multiples of 2^-6 up to 2^22 by default; the gate shapes, the plate and the needle need a finer grid
and say so in Shape.step.  The shapes outside that rule (float bounds beyond float32, |v|^2 outside [1e-100, 1e100], the generic
class) take oracle.cpu_oracle.points_in_box as their yardstick.

Points are laid out in the accepted region's own coordinates: p = c0 + s0 e0 + s1 e1 + s2 e2 with e_a = |v_a|^2 (v_b x v_c) / det the
reciprocal basis scaled so that s in [0, 1]^3 is the region.  For an orthogonal box e_a = v_a; for a sheared one the region is NOT the
corner hull, and points are laid where the two differ.

The camera makes every finite laid-out point valid (depth x + 2^24 in a window (0, inf), a 64 x 32 image): mask 0 is all ones, the
other masks are fixed rectangles, so every count_mb row is the inside matrix summed over a known subset of the points."""
import functools
import itertools
import math
from fractions import Fraction

import numpy as np

import projection_cases as P

W, H = 64, 32
T = np.array([[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [1.0, 0.0, 0.0, 2.0 ** 24], [0.0, 0.0, 0.0, 1.0]])
K = np.array([[W / 2.0, 0.0, W / 2.0], [0.0, H / 2.0, H / 2.0], [0.0, 0.0, 1.0]])
DMIN, DMAX = 0.0, math.inf
LIMIT = 2.0 ** 22
GRID = 64                                             # the default coordinate grid: multiples of 1 / GRID
OTHER = (1, 3, 4)                                     # the corners that span the slabs with corner 0
GATE = 1e-12                                          # the conditioning gate: det^2 > GATE * prod |v_a|^2
M_WIDE = 33


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
def _fr(x):
    return Fraction(float(x))


def _edges(corners):
    """(c0, [v_a], [|v_a|^2]) of finite corners 0, 1, 3, 4 in Fraction"""
    c0 = [_fr(x) for x in corners[0]]
    v = [[_fr(corners[o][i]) - c0[i] for i in range(3)] for o in OTHER]
    return c0, v, [sum(x * x for x in va) for va in v]


@functools.lru_cache(maxsize=None)
def _inside_fraction(cb, pb, oriented):
    c = np.frombuffer(cb, np.float64).reshape(8, 3)
    p = np.frombuffer(pb, np.float32).astype(np.float64)
    if not oriented:
        for k in range(3):
            lo = hi = c[0][k]
            for j in range(1, 8):
                w = c[j][k]
                if w < lo:
                    lo = w
                if w > hi:
                    hi = w
            if not (p[k] >= lo and p[k] <= hi):       # (comparisons of doubles are exact; a NaN fails them)
                return False
        return True
    if not np.all(np.isfinite(p)):
        return False                                  # (p - c0) . v is +-inf or NaN: no quotient of it lies in [0, 1]
    c0, v, vv = _edges(c)
    r = [_fr(p[i]) - c0[i] for i in range(3)]
    for va, w in zip(v, vv):
        if w == 0:
            return False                              # d / 0 is +-inf or NaN
        d = sum(a * b for a, b in zip(r, va))
        if not (0 <= d <= w):
            return False
    return True


def inside_fraction(point, corners, oriented=True):
    """the yardstick: one float32 point (x, y, z) in one box of f64 [8,3] corners (corners 0, 1, 3, 4 finite)"""
    c = np.ascontiguousarray(corners, np.float64).reshape(8, 3)
    assert not oriented or np.all(np.isfinite(c[[0, 1, 3, 4]]))
    return _inside_fraction(c.tobytes(), np.ascontiguousarray(np.asarray(point)[:3], np.float32).tobytes(), bool(oriented))


def slab_margins(point, corners):
    """min over the three slabs of min(|d|, |d - vv|) / vv in Fraction: how far, relative to the slab, the point is from a face"""
    c0, v, vv = _edges(np.asarray(corners, np.float64).reshape(8, 3))
    r = [_fr(point[i]) - c0[i] for i in range(3)]
    out = []
    for va, w in zip(v, vv):
        d = sum(a * b for a, b in zip(r, va))
        out.append(min(abs(d), abs(d - w)) / w)
    return min(out)


def _is_double(r):
    return Fraction(float(r)) == r


def exact_in_double(point, corners):
    """True when the double evaluation of the three slabs is exact for this pair: every difference, product and partial sum (in the
    oracle's order and in NumPy's) and |v_a|^2 is representable, so d and vv are the exact values whatever the summation order"""
    c = np.asarray(corners, np.float64).reshape(8, 3)
    c0, v, vv = _edges(c)
    r = [_fr(point[i]) - c0[i] for i in range(3)]
    vals = list(r) + list(vv)
    for va in v:
        pr = [a * b for a, b in zip(r, va)]
        sq = [a * a for a in va]
        vals += va + pr + sq
        for t in (pr, sq):
            vals += [t[0] + t[1], t[1] + t[2], t[0] + t[2], t[0] + t[1] + t[2]]
    return all(_is_double(x) for x in vals)


def _on_grid(a):
    """elementwise: a finite multiple of 1 / GRID within +-2^22 (then GRID * a is an integer below 2^29)"""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(a) & (np.abs(a) <= LIMIT) & (a * GRID == np.rint(a * GRID))


def inside_matrix(corners, points, oriented=True, generic=()):
    """bool [B, k] of the yardstick.  On-grid (box, point) pairs are evaluated in int64 -- coordinates times 64 are integers below
    2^29, so every product is below 2^58 and every sum below 2^60: exact -- which tests/test_box_table_cases.py holds against
    inside_fraction; every other pair goes through inside_fraction itself.  generic: indices of boxes outside the exactness rule,
    whose rows come from the C oracle."""
    corners = np.asarray(corners, np.float64).reshape(-1, 8, 3)
    pts = np.ascontiguousarray(np.asarray(points, np.float32)[:, :3])
    B, k = len(corners), len(pts)
    out = np.zeros((B, k), bool)
    if not B or not k:
        return out
    p64 = pts.astype(np.float64)
    if not oriented:
        for b, c in enumerate(corners):
            if b in generic:
                continue
            lo, hi = c[0].copy(), c[0].copy()
            for j in range(1, 8):
                lo = np.where(c[j] < lo, c[j], lo)
                hi = np.where(c[j] > hi, c[j], hi)
            with np.errstate(invalid="ignore"):
                out[b] = np.all((p64 >= lo) & (p64 <= hi), axis=1)
    else:
        pg = np.all(_on_grid(p64), axis=1)
        pi = np.where(pg[:, None], np.rint(p64 * GRID), 0).astype(np.int64)
        rest = np.flatnonzero(~pg)
        for b, c in enumerate(corners):
            if b in generic:
                continue
            if np.all(_on_grid(c[[0, 1, 3, 4]])):
                ci = np.rint(c[[0, 1, 3, 4]] * GRID).astype(np.int64)
                r = pi - ci[0]
                ok = pg.copy()
                for a in range(3):
                    va = ci[1 + a] - ci[0]
                    d = r @ va
                    ok &= (d >= 0) & (d <= int(va @ va)) & (int(va @ va) > 0)
                out[b] = ok
                todo = rest
            else:
                todo = range(k)
            for i in todo:
                out[b, i] = inside_fraction(pts[i], c, True)
    if len(generic):
        from oracle import cpu_oracle as orc
        for b in generic:
            out[b] = orc.points_in_box(pts, corners[b], oriented=oriented)
    return out


# ---- the bounds as the box job states them, and two wrong models of them ------------------------------------------------------------------
MODELS = ("stated", "prefilter_by_corner_aabb", "prefilter_without_vv")


def gate_sides(corners):
    """(det^2, 1e-12 * prod |v_a|^2) in double, as the box job writes the conditioning gate"""
    c = np.asarray(corners, np.float64).reshape(8, 3)
    v = [c[o] - c[0] for o in OTHER]
    vv = [float(np.dot(a, a)) for a in v]
    det = float(np.dot(v[0], np.cross(v[1], v[2])))
    return det * det, GATE * (vv[0] * vv[1] * vv[2])


def float_bounds(corners, oriented=True, model="stated"):
    """(lo, hi) float32 [3] bounds of the accepted region with the box job's margin (1e-5 relative + 1e-6), or None for a box it
    leaves unbounded (|v|^2 outside [1e-100, 1e100], the conditioning gate, anything not finite).  model: "stated" -- the reciprocal
    basis e_a = |v_a|^2 (v_b x v_c) / det; "prefilter_by_corner_aabb" -- the extent of corners 0, 1, 3, 4 and their sums;
    "prefilter_without_vv" -- e_a = (v_b x v_c) / det."""
    c = np.asarray(corners, np.float64).reshape(8, 3)
    with np.errstate(all="ignore"):
        if oriented:
            c0 = c[0]
            v = [c[o] - c0 for o in OTHER]
            vv = [float(np.dot(a, a)) for a in v]
            if model == "prefilter_by_corner_aabb":
                e = v
            else:
                if not all(1e-100 <= w <= 1e100 for w in vv):
                    return None
                d2, g = gate_sides(c)
                if not d2 > g:
                    return None
                det = float(np.dot(v[0], np.cross(v[1], v[2])))
                e = [np.cross(v[(a + 1) % 3], v[(a + 2) % 3]) / det * (vv[a] if model == "stated" else 1.0) for a in range(3)]
        else:
            lo, hi = c[0].copy(), c[0].copy()
            for j in range(1, 8):
                lo = np.where(c[j] < lo, c[j], lo)
                hi = np.where(c[j] > hi, c[j], hi)
            c0, e = lo, [np.eye(3)[a] * (hi - lo)[a] for a in range(3)]
        e = np.array(e)
        lov, hiv = c0 + np.minimum(e, 0).sum(0), c0 + np.maximum(e, 0).sum(0)
        if not (np.all(np.isfinite(lov)) and np.all(np.isfinite(hiv))):
            return None
        m = 1e-5 * (np.abs(lov) + np.abs(hiv) + (hiv - lov)) + 1e-6
        return (lov - m).astype(np.float32), (hiv + m).astype(np.float32)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
def corners_of(c0, v1, v2, v3):
    """the 8 corners in the reference's order of use: 0 = c0, 1 = c0 + v1, 3 = c0 + v2, 4 = c0 + v3; 2, 5, 6, 7 the sums"""
    c0, v1, v2, v3 = (np.asarray(x, np.float64) for x in (c0, v1, v2, v3))
    return np.array([c0, c0 + v1, c0 + v1 + v2, c0 + v2, c0 + v3, c0 + v1 + v3, c0 + v1 + v2 + v3, c0 + v2 + v3])


def region_basis(corners):
    """(c0, [e_0, e_1, e_2]) in Fraction, or None for a zero determinant"""
    c0, v, vv = _edges(np.asarray(corners, np.float64).reshape(8, 3))

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    n = [cross(v[(a + 1) % 3], v[(a + 2) % 3]) for a in range(3)]
    det = sum(x * y for x, y in zip(v[0], n[0]))
    if det == 0:
        return None
    return c0, [[vv[a] * x / det for x in n[a]] for a in range(3)]


def _f32(fr):
    """the float32 of a list of Fractions, or None when one is not representable"""
    out = [np.float32(float(x)) for x in fr]
    return out if all(np.isfinite(o) and Fraction(float(o)) == x for o, x in zip(out, fr)) else None


class Shape:
    """one box: name, kind, corners f64 [8,3], points f32 [k,3] with a tag each, step (the grid of its coordinates as a Fraction),
    exact (the exactness rule holds; otherwise the oracle is the yardstick)"""

    def __init__(self, name, kind, corners, step=Fraction(1, GRID), exact=True, layout="region", lattice=None, extra=()):
        self.name, self.kind, self.step, self.exact = name, kind, Fraction(step), exact
        self.corners = np.asarray(corners, np.float64).reshape(8, 3)
        self.points, self.tags = [], []
        if layout == "region":
            self._region()
        elif layout == "one":
            self._one()
        elif layout == "few":
            self._few()
        if lattice is not None:
            for p in lattice:
                self._add([_fr(x) for x in p], "lattice")
        for p, tag in extra:
            self._add([_fr(x) for x in p], tag)
        self.points = np.array(self.points, np.float32).reshape(-1, 3)

    def _add(self, fr, tag, must=True):
        p = _f32(fr)
        if p is None:
            assert not must, (self.name, tag, [float(x) for x in fr])
            return False
        if not all(x / self.step == int(x / self.step) for x in fr) or max(abs(x) for x in fr) > LIMIT:
            assert not must, (self.name, tag, [float(x) for x in fr])
            return False
        self.points.append(p)
        self.tags.append(tag)
        return True

    def _at(self, c0, e, s):
        return [c0[i] + sum(s[a] * e[a][i] for a in range(3)) for i in range(3)]

    def _outside_steps(self, c0, e):
        """one step outside each face, from the face's centre: the smallest power of two that keeps the point on the shape's grid"""
        h = Fraction(1, 2)
        for a in range(3):
            for side in (0, 1):
                for j in range(40, -12, -1):
                    s = [h, h, h]
                    s[a] = -Fraction(2) ** -j if side == 0 else 1 + Fraction(2) ** -j
                    if self._add(self._at(c0, e, s), "out:%d%s" % (a, "-+"[side]), must=False):
                        break
                else:
                    raise AssertionError((self.name, "no outside step", a, side))

    def _region(self):
        c0, e = region_basis(self.corners)
        h = Fraction(1, 2)
        names = {0: "centre", 1: "face", 2: "edge", 3: "vertex"}
        for s in itertools.product((0, h, 1), repeat=3):
            self._add(self._at(c0, e, s), names[sum(1 for x in s if x != h)])
        self._outside_steps(c0, e)
        if self.kind == "sheared":
            _, v, _ = _edges(self.corners)
            hull = [self._at(c0, v, t) for t in itertools.product((0, 1), repeat=3)]
            lo = [min(p[i] for p in hull) for i in range(3)]
            hi = [max(p[i] for p in hull) for i in range(3)]
            q = [Fraction(i, 4) for i in range(5)]
            n = 0
            for s in itertools.product(q, repeat=3):
                p = self._at(c0, e, s)
                if n < 12 and any(p[i] < lo[i] or p[i] > hi[i] for i in range(3)) and self._add(p, "beyond_aabb", must=False):
                    n += 1
            assert n, self.name
            n = 0
            for t in itertools.product((0, h, 1), repeat=3):
                p = self._at(c0, v, t)                    # inside the hull, so inside its AABB
                if n < 12 and not inside_fraction([float(x) for x in p], self.corners) and self._add(p, "aabb_not_region", must=False):
                    n += 1
            assert n, self.name

    def _one(self):
        """the low vertex alone (inside) and a step outside each face"""
        c0, e = region_basis(self.corners)
        self._add(c0, "vertex")
        for a in range(3):
            for s, tag in ((-1, "-"), (2, "+")):
                st = [0, 0, 0]
                st[a] = s
                self._add(self._at(c0, e, st), "out:%d%s" % (a, tag))

    def _few(self):
        """a filler: the centre, the low vertex and one point outside"""
        c0, e = region_basis(self.corners)
        h = Fraction(1, 2)
        self._add(self._at(c0, e, (h, h, h)), "centre")
        self._add(c0, "vertex")
        self._add(self._at(c0, e, (h, h, Fraction(3, 2))), "out:2+")


def _lattice(c0, xs, ys, zs):
    return [(c0[0] + x, c0[1] + y, c0[2] + z) for x in xs for y in ys for z in zs]


CUBOID = ((3, 4, 0), (-4, 3, 0), (0, 0, 5))
TILTED = ((2, 3, 6), (6, -12, 4), (3, 1, -1.5))              # (2,3,6), (3,-6,2), (6,2,-3) are orthogonal: scaled by 1, 2, 1/2
GATE_EPS = (18, 19, 20, 21)                                  # 2^-18 and 2^-19 above the gate (bounded), 2^-20 and 2^-21 below
FAR = 2.0 ** 22 - 144.0


def _replaced(c, value):
    c = np.array(c)
    c[[2, 5, 6, 7]] = value
    return c


@functools.lru_cache(maxsize=None)
def shapes():
    """name -> Shape, the special shapes of the issue"""
    S = []
    add = lambda *a, **k: S.append(Shape(*a, **k))
    add("cuboid", "cuboid", corners_of((10, -3, 1), *CUBOID))
    add("cuboid_tilted", "cuboid", corners_of((-12, 6, 2), *TILTED))
    add("cuboid_left", "cuboid", corners_of((10, 9, 1), CUBOID[1], CUBOID[0], CUBOID[2]))
    add("cuboid_permuted", "cuboid", corners_of((20, -3, 1), CUBOID[1], CUBOID[2], CUBOID[0]))
    add("cuboid_tilted_left", "cuboid", corners_of((-12, -14, 2), TILTED[2], TILTED[1], TILTED[0]))
    add("shear1", "sheared", corners_of((8, -20, 1), (4, 0, 0), (4, 4, 0), (0, 0, 4)))
    add("shear2", "sheared", corners_of((18, -20, 1), (4, 0, 0), (4, 4, 0), (0, 4, 4)))
    add("shear3", "sheared", corners_of((28, -20, 1), (4, 0, 4), (4, 4, 0), (0, 4, 4)))
    add("shear_negative", "sheared", corners_of((-20, -12, -2), (-4, 0, 0), (-4, -4, 0), (0, -4, -4)))
    add("shear2_left", "sheared", corners_of((18, -30, 1), (4, 4, 0), (4, 0, 0), (0, 4, 4)))
    zs = [0.0] + [s * 2.0 ** k for k in (10, 19, 20, 21) for s in (1, -1)]
    for k in GATE_EPS:
        c0 = (30.0, 8.0 * (k - 18), 0.0)
        add("gate_2^-%d" % k, "gate", corners_of(c0, (4, 0, 0), (0, 4, 0), (4, 0, 4 * 2.0 ** -k)), step=Fraction(1, 2 ** (k - 2)),
            layout=None, lattice=_lattice(c0, (-1, 0, 1, 2, 3, 4, 5), (-1, 0, 2, 4, 5), zs))
    c0 = (-30.0, 8.0, 0.0)
    add("prism", "prism", corners_of(c0, (4, 0, 0), (0, 4, 0), (4, 0, 0)), layout=None,
        lattice=_lattice(c0, (-1, 0, 2, 4, 5), (-1, 0, 2, 4, 5), [0.0] + [s * 2.0 ** k for k in (10, 20) for s in (1, -1)]))
    a, t = 2.0 ** 13, 2.0 ** -7
    add("plate", "thin", corners_of((-2.0 ** 14, -2.0 ** 14, 0), (3 * a, 4 * a, 0), (-4 * a, 3 * a, 0), (0, 0, 5 * t)), step=Fraction(1, 256))
    add("needle", "thin", corners_of((0, 40, 0), (3 * a, 4 * a, 0), (-4 * t, 3 * t, 0), (0, 0, 5 * t)), step=Fraction(1, 256))
    g = 1.0 / GRID
    add("tiny", "tiny", corners_of((5, 5, 1), (g, 0, 0), (0, g, 0), (0, 0, g)), layout="one")
    b = 2.0 ** 21
    add("big", "big", corners_of((-b / 2, -b / 2, -b / 2), (b, 0, 0), (0, b, 0), (0, 0, b)), step=Fraction(1, 8))
    add("far", "far", corners_of((FAR, FAR, 0), (16, 0, 0), (0, 16, 0), (0, 0, 16)), step=Fraction(1, 4))
    base = corners_of((-6, -30, 1), *CUBOID)
    between = [((1000, 1000, 1000), "between"), ((2.0 ** 21, 2.0 ** 21, 2.0 ** 21), "between"), ((-7, -30, 1), "between")]
    add("replaced_far", "replaced", _replaced(base, LIMIT), extra=between)
    add("replaced_nan", "replaced", _replaced(corners_of((4, -30, 1), *CUBOID), np.nan), extra=between)
    # outside the exactness rule: the oracle is the yardstick
    lat = _lattice((0, 0, 0), (-3, -2, 0, 2, 3, 2.0 ** 20), (-3, -2, 0, 2, 3), (-3, -2, 0, 2, 3, -2.0 ** 20))
    add("overflow", "overflow", corners_of((-2, -2, -2), (1e39, 0, 0), (0, 1e39, 0), (0, 0, 1e39)), exact=False, layout=None, lattice=lat)
    add("overflow_negative", "overflow", corners_of((2, 2, 2), (-1e39, 0, 0), (0, -1e39, 0), (0, 0, -1e39)), exact=False, layout=None, lattice=lat)
    add("vv_huge", "vv", corners_of((-2, -2, -2), (1e60, 0, 0), (0, 1e60, 0), (0, 0, 1e60)), exact=False, layout=None, lattice=lat)
    tiny = [(0, 0, 0), (g, 0, 0), (-g, 0, 0), (0, g, 0), (0, -g, 0), (0, 0, g), (0, 0, -g)]
    add("vv_tiny", "vv", corners_of((0, 0, 0), (1e-60, 0, 0), (0, 1e-60, 0), (0, 0, 1e-60)), exact=False, layout=None, lattice=tiny)
    return {s.name: s for s in S}


FILLER_EDGES = (((4, 0, 0), (0, 2, 0), (0, 0, 1.5)), ((1.5, 2, 0), (-4, 3, 0), (0, 0, 1.5)), ((0, 2, 0), (-4, 0, 0), (0, 0, 2)),
                ((-2, 1.5, 0), (-3, -4, 0), (0, 0, 1.5)))
UNIT_EDGES = (((1, 0, 0), (0, 1, 0), (0, 0, 1)), ((0, 1, 0), (-1, 0, 0), (0, 0, 1)), ((0, 0, 1), (1, 0, 0), (0, 1, 0)),
              ((-1, 0, 0), (0, 0, -1), (0, -1, 0)))


@functools.lru_cache(maxsize=None)
def filler(j, unit=False, full=False):
    """upright, car-sized cuboids on a 6 m raster (what the suite sent through the tables before); unit: unit cubes, axes permuted"""
    e = (UNIT_EDGES if unit else FILLER_EDGES)[j % 4]
    c0 = (6.0 + 6 * (j % 12) - 36, -33.0 + 6 * (j // 12), 0.5 * (j % 3))
    return Shape("%s%d" % ("unit" if unit else "filler", j), "cuboid", corners_of(c0, *e), layout="region" if full else "few")


@functools.lru_cache(maxsize=None)
def unbounded_filler(j):
    """an infinite prism (v3 == v1) of its own place: the box job leaves it unbounded"""
    c0 = (6.0 * (j % 12) - 30, 6.0 * (j // 12) - 30, 0.0)
    return Shape("prism%d" % j, "prism", corners_of(c0, (4, 0, 0), (0, 4, 0), (4, 0, 0)), layout=None,
                 lattice=[(c0[0] + 2, c0[1] + 2, 2.0 ** 20), (c0[0] + 2, c0[1] + 5, 0.0), (c0[0], c0[1], -2.0 ** 10)])


# ---- the camera and the masks -----------------------------------------------------------------------------------------------------------------
_pix = {}


def pixel(p):
    """(u, v, valid) of one float32 point under the camera, by the exact restatement of the projection"""
    key = np.asarray(p, np.float32)[:3].tobytes()
    if key not in _pix:
        x = [float(t) for t in np.frombuffer(key, np.float32)]
        uf, vf, d = P.exact_project(x, T, K)
        ru, rv = P.rint(uf), P.rint(vf)
        ok = (ru >= 0) and (ru < W) and (rv >= 0) and (rv < H) and (d > DMIN) and (d < DMAX)
        _pix[key] = (int(ru) if ok else -1, int(rv) if ok else -1, bool(ok))
    return _pix[key]


RECTS = ((0, 0, W, H), (32, 16, 33, 17), (0, 0, 32, H), (33, 0, W, H), (0, 0, W, 16), (0, 17, W, H), (30, 14, 35, 19), (0, 0, 0, 0),
         (32, 16, W, H))                                     # (u0, v0, u1, v1), half open; mask 0 is the whole image, mask 7 is empty


def masks(M):
    """uint8 [M, H, W]: mask m is the rectangle RECTS[m % 9]; mask 32 of the wide set is all ones again"""
    out = np.zeros((M, H, W), np.uint8)
    for m in range(M):
        u0, v0, u1, v1 = RECTS[0] if m == 32 else RECTS[m % len(RECTS)]
        out[m, v0:v1, u0:u1] = 1
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------------
NONFINITE = np.array([[np.nan, 1, 1], [np.inf, 1, 1], [-np.inf, 1, 1]], np.float32)


class Scene:
    """one frame: boxes (Shapes), their corners [B,8,3], the points f32 [N,4] (every box's own, then per word the grid-border points
    and points outside its domain, then NaN, +inf and -inf in x), owner [N] (the box a point was laid for, or -1), tags, and ``special``
    {box index: shape name}.  Everything derived is computed once and must not be written to."""

    def __init__(self, name, boxes, special, kind):
        self.name, self.boxes, self.special, self.kind = name, list(boxes), dict(special), kind
        B = len(self.boxes)
        self.corners = np.array([s.corners for s in self.boxes]).reshape(B, 8, 3)
        self.generic = tuple(b for b, s in enumerate(self.boxes) if not s.exact)
        pts, owner, tags = [], [], []
        for b, s in enumerate(self.boxes):
            pts.append(s.points)
            owner += [b] * len(s.points)
            tags += s.tags
        for w in range((B + 63) // 64):
            bp = self.border_points(w)
            pts.append(bp)
            owner += [-1] * len(bp)
            tags += ["border:%d" % w] * len(bp)
        pts.append(NONFINITE)
        owner += [-1] * 3
        tags += ["nonfinite"] * 3
        xyz = np.concatenate(pts).astype(np.float32)
        self.points = np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], axis=1)
        self.owner, self.tags = np.array(owner), tags
        self._cache = {}

    def domain(self, w, oriented=True):
        """(x0, y0, x1, y1) float32: the extent of the float bounds of word w's bounded boxes, or None"""
        bs = [float_bounds(c, oriented) for c in self.corners[64 * w:64 * w + 64]]
        bs = [b for b in bs if b is not None and np.all(np.isfinite(b[0])) and np.all(np.isfinite(b[1]))]
        if not bs:
            return None
        lo, hi = np.min([b[0] for b in bs], axis=0), np.max([b[1] for b in bs], axis=0)
        return lo[0], lo[1], hi[0], hi[1]

    def border_points(self, w):
        """points whose x or y equals a float bound of word w's domain (and the floats next to it), and points 8 m outside the domain
        on all four sides, at the heights 1 and 2^20 (the second inside the unbounded shapes); a word without a domain: around 0"""
        d = self.domain(w) or (np.float32(-8), np.float32(-8), np.float32(8), np.float32(8))
        x0, y0, x1, y1 = d
        xm, ym = np.float32((float(x0) + float(x1)) / 2), np.float32((float(y0) + float(y1)) / 2)
        out = []
        f = np.float32
        for z in (1.0, 2.0 ** 20):
            for x in (x0, np.nextafter(x0, f(-np.inf)), np.nextafter(x0, f(np.inf)), x1, np.nextafter(x1, f(np.inf)), np.nextafter(x1, f(-np.inf)),
                      x0 - f(8), x1 + f(8)):
                out.append((x, ym, z))
            for y in (y0, np.nextafter(y0, f(-np.inf)), np.nextafter(y0, f(np.inf)), y1, np.nextafter(y1, f(np.inf)), np.nextafter(y1, f(-np.inf)),
                      y0 - f(8), y1 + f(8)):
                out.append((xm, y, z))
            out += [(x0 - f(8), y0 - f(8), z), (x1 + f(8), y1 + f(8), z)]
        out = np.array(out, np.float32)
        return out[np.all(np.abs(out) <= LIMIT, axis=1)]

    def _get(self, key, fn):
        if key not in self._cache:
            v = fn()
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            self._cache[key] = v
        return self._cache[key]

    def inside(self, oriented=True):
        return self._get(("inside", bool(oriented)), lambda: inside_matrix(self.corners, self.points, oriented, self.generic))

    def pixels(self):
        """(u [N], v [N], valid [N])"""
        def fn():
            t = [pixel(p) for p in self.points]
            return np.array([a for a, _, _ in t]), np.array([b for _, b, _ in t]), np.array([c for _, _, c in t], bool)
        return self._get("pix", fn)

    def member(self, M):
        """bool [M, N]: point n is valid and its pixel lies in mask m"""
        def fn():
            u, v, ok = self.pixels()
            mk = masks(M)
            out = np.zeros((M, len(u)), bool)
            out[:, ok] = mk[:, v[ok], u[ok]] != 0
            return out
        return self._get(("member", M), fn)

    def expected(self, M, oriented=True, within=None):
        """dict(count_mb int64 [M, B], best_box int32 [M], best_cnt int64 [M]); within: a bool [B, N] a prefilter model adds"""
        ins = self.inside(oriented)
        if within is not None:
            ins = ins & within
        cnt = self.member(M).astype(np.int64) @ ins.T.astype(np.int64)
        return dict(count_mb=cnt.reshape(M, len(self.boxes)), **first_strict_maximum(cnt.reshape(M, len(self.boxes))))


def first_strict_maximum(count_mb):
    """best_box / best_cnt as the reference picks them: the first box whose count exceeds every earlier one, from 0 (none: -1, 0)"""
    M = count_mb.shape[0]
    bb, bc = np.full(M, -1, np.int32), np.zeros(M, np.int64)
    for m in range(M):
        for b, c in enumerate(count_mb[m]):
            if c > bc[m]:
                bc[m], bb[m] = c, b
    return dict(best_box=bb, best_cnt=bc)


def model_within(scene, model, oriented=True):
    """bool [B, N]: the (box, point) pairs a kernel would still test exactly if its float bounds were ``model``'s"""
    p = scene.points[:, :3]
    out = np.ones((len(scene.boxes), len(p)), bool)
    for b, c in enumerate(scene.corners):
        fb = float_bounds(c, oriented, model)
        if fb is not None:
            with np.errstate(invalid="ignore"):
                out[b] = np.all((p >= fb[0]) & (p <= fb[1]), axis=1)
    return out


def model_counts(scene, model, M, oriented=True):
    """the count_mb a kernel with that prefilter would give"""
    return scene.expected(M, oriented, model_within(scene, model, oriented))["count_mb"]


def _assemble(name, B, special, kind, unit=False, unbounded_word=None):
    sh = shapes()
    boxes, j = [], 0
    for b in range(B):
        if b in special:
            boxes.append(sh[special[b]])
        elif unbounded_word is not None and b // 64 == unbounded_word:
            boxes.append(unbounded_filler(b))
        else:
            boxes.append(filler(j, unit, full=(j < 2)))
            j += 1
    return Scene(name, boxes, special, kind)


def _spread(names, B):
    """the special shapes at 0, 63, 64 and the last box first, the rest behind them"""
    slots = [b for b in (0, 63, 64, B - 1) if b < B]
    slots = sorted(set(slots), key=slots.index) + [b for b in range(1, B) if b not in (0, 63, 64, B - 1)]
    return dict(zip(slots, names))


SHEARED = ("shear1", "shear2", "shear3", "shear_negative", "shear2_left")
CUBOIDS = ("cuboid", "cuboid_tilted", "cuboid_left", "cuboid_permuted", "cuboid_tilted_left")


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> Scene.  Box counts 1, 63, 64, 65 and 129; kind "sheared" scenes hold sheared shapes, "cuboid" scenes only orthogonal
    boxes (what the suite had before), "mixed" the rest"""
    sh = shapes()
    S = [
        _assemble("one", 1, {0: "shear2"}, "sheared"),
        _assemble("b63", 63, _spread(("shear3", "gate_2^-19", "tiny", "plate", "replaced_nan"), 63), "sheared"),
        _assemble("b64", 64, _spread(("shear_negative", "far", "gate_2^-20", "needle", "replaced_far"), 64), "sheared"),
        _assemble("b65", 65, _spread(("shear1", "gate_2^-18", "prism", "big", "overflow", "vv_tiny"), 65), "sheared"),
        _assemble("b129", 129, _spread(("shear2", "shear2_left", "shear3", "shear_negative") + tuple(
            n for n in sh if n not in ("shear2", "shear2_left", "shear3", "shear_negative", "far", "big")), 129), "sheared"),
        # word 1 (boxes 64..127) holds unbounded boxes only: its domain is empty
        _assemble("b129_unbounded_word", 129, {0: "shear1", 63: "cuboid", 64: "gate_2^-21", 65: "vv_huge", 66: "prism", 127: "gate_2^-20",
                                               128: "shear3"}, "sheared", unbounded_word=1),
        _assemble("b5", 5, {0: "cuboid_tilted", 4: "shear2"}, "sheared"),
        _assemble("cuboids", 65, _spread(CUBOIDS, 65), "cuboid"),
        _assemble("unit_cuboids", 65, {}, "cuboid", unit=True),
        Scene("empty", [], {}, "cuboid"),
    ]
    return {s.name: s for s in S}


BATCH3 = ("b129", "empty", "b5")                             # F = 3 with 129, 0 and 5 boxes: the per-frame table path
M_OF = {"b129": 9}                                           # 9 x 129 = 1161 count_mb entries, above the 1024 that finalize stages


def masks_of(name):
    return M_OF.get(name, 3)


# ---- the generic class ----------------------------------------------------------------------------------------------------------------------------
GENERIC_BOXES, GENERIC_POINTS, GENERIC_FRAMES = 256, 64, 2
MARGIN = Fraction(1, 2 ** 30)


def _generic_box(rng):
    """c0 and three edges of 0.1 .. 100 m along unit directions whose matrix has a condition number up to 1e5"""
    while True:
        q1, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        q2, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        s = 10.0 ** -rng.uniform(0, 5, 2)
        n = q1 @ np.diag([1.0, s[0], s[0] * s[1]]) @ q2.T
        n /= np.linalg.norm(n, axis=0)
        if np.linalg.cond(n) <= 1e5:
            break
    v = (n * 10.0 ** rng.uniform(-1, 2, 3)).T
    centre = rng.uniform(-200, 200, 3)
    return corners_of(centre - v.sum(0) / 2, *v)


def _margins_double(p, corners):
    """[B, k] of min(|d|, |d - vv|) / vv in double, vectorised: a screen for the Fraction rule"""
    c0 = corners[:, 0]
    out = np.full((len(corners), len(p)), np.inf)
    for o in OTHER:
        v = corners[:, o] - c0
        vv = np.einsum("bi,bi->b", v, v)
        d = np.einsum("bi,ki->bk", v, p) - np.einsum("bi,bi->b", v, c0)[:, None]
        out = np.minimum(out, np.minimum(np.abs(d), np.abs(d - vv[:, None])) / vv[:, None])
    return out


@functools.lru_cache(maxsize=None)
def generic():
    """GENERIC_FRAMES frames of seeded parallelepipeds with arbitrary double entries, each with 64 float32 points drawn around its
    region (in the region's coordinates where they stay within 2^21, around the corner hull otherwise).  A point is redrawn while some
    slab of its own box has |d| / vv or |d - vv| / vv below 2^-30 in Fraction, or while the double screen puts it within 2^-26 of a face
    of any box of its frame.  Returns a list of dict(corners [B,8,3], points f32 [N,4], owner [N])."""
    rng = np.random.default_rng(20240611)
    per = GENERIC_BOXES // GENERIC_FRAMES
    frames = []
    for f in range(GENERIC_FRAMES):
        corners = np.array([_generic_box(rng) for _ in range(per)])
        pts, owner = [], []
        for b, c in enumerate(corners):
            v = np.array([c[o] - c[0] for o in OTHER])
            vv = (v * v).sum(1)
            det = np.dot(v[0], np.cross(v[1], v[2]))
            e = np.array([np.cross(v[(a + 1) % 3], v[(a + 2) % 3]) * vv[a] / det for a in range(3)])
            n = 0
            while n < GENERIC_POINTS:
                mode = n % 4
                s = rng.uniform(0, 1, 3) if mode == 0 else rng.uniform(-0.5, 1.5, 3)
                if mode == 2:                                # next to a face of the region
                    a = rng.integers(3)
                    s[a] = rng.choice([0.0, 1.0]) + rng.choice([-1, 1]) * 10.0 ** -rng.uniform(2, 6)
                p = c[0] + s @ (v if mode == 3 else e)
                if not np.all(np.abs(p) <= 2.0 ** 21):
                    p = c[0] + s @ v
                p = p.astype(np.float32)
                if _margins_double(p[None].astype(np.float64), corners).min() < 2.0 ** -26 or slab_margins(p, c) < MARGIN:
                    continue
                pts.append(p)
                owner.append(b)
                n += 1
        xyz = np.array(pts, np.float32)
        frames.append(dict(corners=corners, points=np.concatenate([xyz, np.zeros((len(xyz), 1), np.float32)], axis=1), owner=np.array(owner)))
    return frames


def generic_inside(frame, oriented=True):
    """bool [B, N] by the C oracle, the generic class's yardstick"""
    from oracle import cpu_oracle as orc
    return np.array([orc.points_in_box(frame["points"], c, oriented=oriented) for c in frame["corners"]])


# ---- the checker -----------------------------------------------------------------------------------------------------------------------------------
def word_of(b):
    return b // 64


def describe(scene, b, i=None):
    s = "scene %s, box %d (%s, word %d)" % (scene.name, b, scene.boxes[b].name, word_of(b))
    if i is not None:
        s += ", point %d %s [%s, laid for box %d]" % (i, scene.points[i, :3].tolist(), scene.tags[i], scene.owner[i])
    return s


def check_counts(scene, path, got, M, oriented=True, keys=("count_mb", "best_box", "best_cnt")):
    """got: dict with count_mb [M, B] (and best_box, best_cnt [M]) of one frame: integer equality with the yardstick, and a message
    that names the scene, shape, box index, word, path and the first point of that box and mask the result may have missed"""
    want = scene.expected(M, oriented)
    B = len(scene.boxes)
    for k in keys:
        g = np.asarray(got[k]).reshape(want[k].shape).astype(np.int64)
        if np.array_equal(g, want[k]):
            continue
        if k != "count_mb":
            m = int(np.flatnonzero(g != want[k])[0])
            raise AssertionError("%s: %s, oriented=%d: %s of mask %d is %d, expected %d" % (path, scene.name, oriented, k, m, g[m], want[k][m]))
        m, b = (int(x) for x in np.argwhere(g != want[k])[0])
        ins = scene.inside(oriented)[b] & scene.member(M)[m]
        within = model_within(scene, "stated", oriented)[b]
        first = np.flatnonzero(ins & ~within) if np.any(ins & ~within) else np.flatnonzero(ins)
        i = int(first[0]) if len(first) else None
        raise AssertionError("%s: oriented=%d, mask %d, %s: count %d, expected %d (%d boxes differ); first inside point%s: %s"
                             % (path, oriented, m, describe(scene, b), g[m, b], want[k][m, b], int(np.count_nonzero((g != want[k]).any(0))),
                                " outside the stated float bounds" if np.any(ins & ~within) else "", describe(scene, b, i) if i is not None else "none"))
    assert B == want["count_mb"].shape[1]


def check_inside(scene, path, got, oriented=True):
    """got: bool [B, N] against the inside matrix; names the first differing point"""
    want = scene.inside(oriented)
    got = np.asarray(got).astype(bool).reshape(want.shape)
    if not np.array_equal(got, want):
        b, i = (int(x) for x in np.argwhere(got != want)[0])
        raise AssertionError("%s: oriented=%d, %s: inside is %s, expected %s (%d pairs differ)"
                             % (path, oriented, describe(scene, b, i), got[b, i], want[b, i], int(np.count_nonzero(got != want))))


def pair_census(scene, M=None, oriented=True):
    """how many (point, box) pairs a check of this scene covers, and how many of them are of the kinds the tables could get wrong"""
    ins = scene.inside(oriented)
    n = dict(pairs=ins.size, inside=int(ins.sum()), beyond_corner_aabb=0, on_face=0, in_unbounded_box=0, beyond_first_word=int(ins[64:].size),
             inside_beyond_first_word=int(ins[64:].sum()))
    corner = model_within(scene, "prefilter_by_corner_aabb", oriented)
    n["beyond_corner_aabb"] = int((ins & ~corner).sum())
    for b, s in enumerate(scene.boxes):
        if float_bounds(s.corners, oriented) is None:
            n["in_unbounded_box"] += int(ins[b].sum())
        own = scene.owner == b
        n["on_face"] += int(sum(1 for i in np.flatnonzero(own) if scene.tags[i] in ("vertex", "edge", "face") and ins[b, i]))
    return n
