"""The rectangular linear sum assignment of lpf_assign_costs / lpf_assign_2d restated in plain Python: shortest augmenting paths with
duals, statement for statement what scipy.optimize.linear_sum_assignment runs, with the column choice written as the order-independent
rule a parallel reduction needs.  It is the yardstick where SciPy's version differs, and the documentation of the tie rule:

  among the positions of `remaining` whose shortest path cost equals the minimum, the LAST one whose column is free; if none is free,
  the FIRST one.

That is the closed form of SciPy's sequential scan `if spc[j] < lowest or (spc[j] == lowest and row4col[j] == -1): index = it`: a
strictly lower value always takes over, an equal one only when its column is free -- so the scan ends on the last free column among the
equals, or, when none of them is free, on the position that first brought the minimum.  `remaining` is filled DESCENDING (nc - 1 .. 0)
and a chosen position is overwritten with the last one: both decide which of several equal columns is met first, so both are kept.

solve(cost) -> (status, rows, cols): 0 solved, 1 invalid entries (NaN or -inf), 2 infeasible.  cases(): the seeded case list the CPU
and GPU tests and tests/golden/make_golden_assign.py share."""
import numpy as np

OK, INVALID, INFEASIBLE = 0, 1, 2
CAP = 1024                        # LPF_ASSIGN_MAX


def _argmin(vals, free):
    """the rule above for the values / free flags of remaining[0 .. n_rem): keyed on (value, free?, position), order-independent"""
    low = vals.min()
    at = np.flatnonzero(vals == low)
    fr = at[free[at]]
    return int(fr[-1]) if len(fr) else int(at[0])


def _argmin_scan(vals, free):
    """SciPy's sequential scan (the rule's definition)"""
    index, lowest = -1, np.inf
    for it in range(len(vals)):
        if vals[it] < lowest or (vals[it] == lowest and free[it]):
            lowest, index = vals[it], it
    return index


def solve(cost, argmin=_argmin, first_min=False, ascending=False):
    """(status, rows int64, cols int64) of a [D,B] float64 matrix.  first_min / ascending: the two WRONG variants the tests show to
    disagree with SciPy (first minimum among equals; `remaining` filled ascending)."""
    cost = np.asarray(cost, np.float64)
    D, B = cost.shape
    none = np.zeros(0, np.int64)
    if D == 0 or B == 0:
        return OK, none, none
    if np.isnan(cost).any() or (cost == -np.inf).any():
        return INVALID, none, none
    tall = B < D
    c = np.ascontiguousarray(cost.T) if tall else cost
    nr, nc = c.shape
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1, np.int64), np.full(nc, -1, np.int64)
    path = np.full(nc, -1, np.int64)
    for cur in range(nr):
        min_val, i = 0.0, cur
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        spc = np.full(nc, np.inf)
        remaining = np.arange(nc) if ascending else np.arange(nc - 1, -1, -1)
        n_rem = nc
        sink = -1
        for _ in range(nc):                                  # bounded by n_rem: a step removes one column
            SR[i] = True
            js = remaining[:n_rem]
            r = ((min_val + c[i, js]) - u[i]) - v[js]        # in exactly this order
            better = r < spc[js]
            spc[js[better]] = r[better]
            path[js[better]] = i
            vals, free = spc[js], row4col[js] == -1
            index = int(np.argmin(vals)) if first_min else argmin(vals, free)
            min_val = spc[remaining[index]]
            if min_val == np.inf:
                return INFEASIBLE, none, none
            j = remaining[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            n_rem -= 1
            remaining[index] = remaining[n_rem]
            if sink >= 0:
                break
        if sink < 0:
            return INFEASIBLE, none, none
        u[cur] += min_val
        for k in np.flatnonzero(SR):
            if k != cur:
                u[k] += min_val - spc[col4row[k]]
        sc = np.flatnonzero(SC)
        v[sc] -= min_val - spc[sc]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if tall:
        order = np.argsort(col4row, kind="stable")
        return OK, col4row[order].astype(np.int64), order.astype(np.int64)
    return OK, np.arange(nr, dtype=np.int64), col4row.astype(np.int64)


def solve_front(cost, front):
    """solve() on the columns with front != 0 (V5:337-341), the columns in ORIGINAL numbering"""
    cost = np.asarray(cost, np.float64)
    if front is None:
        return solve(cost)
    live = np.flatnonzero(np.asarray(front) != 0)
    st, rows, cols = solve(cost[:, live])
    return st, rows, live[cols].astype(np.int64)


# ---- the seeded case list ------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 5), (5, 1), (3, 3), (7, 12), (12, 7), (63, 64), (64, 64), (64, 65), (65, 64), (64, 129), (130, 70), (1024, 1000))
KINDS = ("int012", "constant", "repeated_row", "one_minus_f32", "decimal")
LARGE_KINDS = ("int012", "one_minus_f32")         # the kinds of the shape at the cap (a test stays within seconds)


def matrix(rng, kind, D, B):
    if kind == "int012":
        return rng.integers(0, 3, (D, B)).astype(np.float64)
    if kind == "constant":
        return np.full((D, B), 0.75)
    if kind == "repeated_row":
        m = np.repeat(rng.random((1, B)), D, axis=0)
        m[rng.random((D, B)) < 0.2] = 0.5
        return m
    if kind == "one_minus_f32":
        return 1.0 - rng.random((D, B), dtype=np.float32).astype(np.float64)
    if kind == "decimal":
        m = np.round(rng.random((D, B)), 1)
        m[rng.random((D, B)) < 0.3] = 1.0
        return m
    raise ValueError(kind)


def cases():
    """[(name, [D,B] float64)] in a fixed order from ONE default_rng(0)"""
    rng = np.random.default_rng(0)
    out = []
    for D, B in SHAPES:
        for kind in (LARGE_KINDS if max(D, B) > 256 else KINDS):
            out.append(("%s_%dx%d" % (kind, D, B), matrix(rng, kind, D, B)))
    return out


def small_cases(n, seed=1):
    """n seeded small matrices of four kinds (wide, tall and square up to 9 x 9) for the comparison with SciPy"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        D, B = int(rng.integers(1, 10)), int(rng.integers(1, 10))
        out.append(matrix(rng, ("int012", "repeated_row", "one_minus_f32", "decimal")[k % 4], D, B))
    return out
