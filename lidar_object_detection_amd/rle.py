"""Run-length masks: one frame's instance masks as runs of member pixels (LpfContext.set_masks_rle, lpf_set_masks_rle).

A run is ``(start, length)``: the pixels ``start .. start + length - 1`` of the mask image flattened row-major (pixel (x, y) is
``y * W + x``).  Mask m owns ``runs[run_off[m]:run_off[m + 1]]``.  A pixel is a member iff it lies in any run of its mask; the runs
this module produces are canonical (ascending, maximal: no two touch), the library accepts any order and overlaps."""
import numpy as np


def _runs_of(flat):
    """Canonical runs [R,2] int32 of a flat bool vector."""
    d = np.diff(np.concatenate(([0], flat.view(np.int8), [0])))
    start = np.flatnonzero(d == 1)
    end = np.flatnonzero(d == -1)
    return np.stack([start, end - start], axis=1).astype(np.int32).reshape(-1, 2)


def check_runs(runs, run_off, n_masks, hw, who="RleMasks"):
    """(runs int32 [R,2], run_off int64 [n_masks + 1]) as the library takes them; ValueError for another dtype or shape, an offset table
    that does not start at 0, decreases or does not end at R, and a run with start < 0, length < 0 or start + length > hw."""
    r = np.asarray(runs)
    o = np.asarray(run_off)
    if r.dtype.kind not in "iu" or o.dtype.kind not in "iu":
        raise ValueError("%s: runs and run_off must be integer arrays, got %s and %s" % (who, r.dtype, o.dtype))
    if r.ndim != 2 or r.shape[1] != 2:
        raise ValueError("%s: runs must be [R,2] (start, length), got %s" % (who, r.shape))
    if o.shape != (n_masks + 1,):
        raise ValueError("%s: run_off must be [%d], got %s" % (who, n_masks + 1, o.shape))
    o = o.astype(np.int64)
    if o[0] != 0 or (np.diff(o) < 0).any() or o[-1] != len(r):
        raise ValueError("%s: run_off must start at 0, never decrease and end at the number of runs (%d)" % (who, len(r)))
    r64 = r.astype(np.int64)
    bad = np.flatnonzero((r64[:, 0] < 0) | (r64[:, 1] < 0) | (r64[:, 0] + r64[:, 1] > hw))
    if len(bad):
        k = int(bad[0])
        raise ValueError("%s: mask %d run %d: start=%d length=%d (0 <= start, 0 <= length, start + length <= H*W = %d)"
                         % (who, int(np.searchsorted(o, k, side="right")) - 1, k - int(o[np.searchsorted(o, k, side="right") - 1]),
                            r64[k, 0], r64[k, 1], hw))
    return np.ascontiguousarray(r64.astype(np.int32)), np.ascontiguousarray(o)


class RleMasks:
    """One frame's masks in run-length form: ``runs`` int32 [R,2], ``run_off`` int64 [M + 1], ``shape == (M, H, W)``."""

    def __init__(self, runs, run_off, shape):
        M, H, W = (int(v) for v in shape)
        if M < 0 or H <= 0 or W <= 0:
            raise ValueError("RleMasks: shape must be (M, H, W) with M >= 0 and H, W > 0, got %s" % (tuple(shape),))
        self.runs, self.run_off = check_runs(runs, run_off, M, H * W)
        self.shape = (M, H, W)

    @classmethod
    def from_dense(cls, masks, rule="nonzero"):
        """masks [M,H,W] uint8 / bool / float -> canonical runs.  rule: "nonzero" (member <=> value != 0) or, for float masks, "gt0.5"
        (member <=> value > 0.5, as Same_color.py:125 reads a detector's float masks)."""
        a = np.asarray(masks)
        if a.ndim != 3:
            raise ValueError("from_dense: masks must be [M,H,W], got %s" % (a.shape,))
        if rule == "nonzero":
            member = a != 0
        elif rule == "gt0.5":
            if a.dtype.kind != "f":
                raise ValueError('from_dense: rule "gt0.5" is for float masks, got %s' % a.dtype)
            member = a > 0.5
        else:
            raise ValueError('from_dense: rule must be "nonzero" or "gt0.5", got %r' % (rule,))
        M, H, W = a.shape
        if H <= 0 or W <= 0:
            raise ValueError("from_dense: empty image %s" % (a.shape,))
        per = [_runs_of(np.ascontiguousarray(member[m]).reshape(-1)) for m in range(M)]
        off = np.zeros(M + 1, np.int64)
        off[1:] = np.cumsum([len(p) for p in per])
        runs = np.concatenate(per) if per else np.zeros((0, 2), np.int32)
        return cls(runs, off, (M, H, W))

    @classmethod
    def from_coco(cls, counts_per_mask, H, W):
        """COCO's UNCOMPRESSED counts, one list per mask: column-major, alternating lengths of zeros and ones, beginning with the zeros
        (``{"size": [H, W], "counts": [...]}``).  The compressed string form is not read.  Goes through a dense image on the host."""
        H, W = int(H), int(W)
        dense = np.zeros((len(counts_per_mask), H, W), np.uint8)
        for m, counts in enumerate(counts_per_mask):
            c = np.asarray(counts)
            if c.ndim != 1 or (len(c) and c.dtype.kind not in "iu") or (c < 0).any() or int(c.sum()) != H * W:
                raise ValueError("from_coco: mask %d: counts must be non-negative integers that sum to H*W = %d" % (m, H * W))
            col = np.zeros(H * W, np.uint8)
            edges = np.concatenate(([0], np.cumsum(c.astype(np.int64))))
            for i in range(1, len(c), 2):
                col[edges[i]:edges[i + 1]] = 1
            dense[m] = col.reshape(W, H).T
        return cls.from_dense(dense)

    def to_dense(self):
        """uint8 [M,H,W], 1 = member."""
        M, H, W = self.shape
        out = np.zeros((M, H * W), np.uint8)
        for m in range(M):
            r = self.runs[self.run_off[m]:self.run_off[m + 1]].astype(np.int64)
            d = np.zeros(H * W + 1, np.int64)
            np.add.at(d, r[:, 0], 1)
            np.add.at(d, r[:, 0] + r[:, 1], -1)
            out[m] = np.cumsum(d[:-1]) > 0
        return out.reshape(M, H, W)

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError("RleMasks takes slices over masks (rle[a:b]), got %r" % (key,))
        a, b, step = key.indices(self.shape[0])
        if step != 1:
            raise TypeError("RleMasks slices have step 1")
        b = max(a, b)
        lo, hi = int(self.run_off[a]), int(self.run_off[b])
        return RleMasks(self.runs[lo:hi], self.run_off[a:b + 1] - lo, (b - a,) + self.shape[1:])

    def __array__(self, *args, **kwargs):
        raise TypeError("RleMasks is not an array: use .to_dense() for entry points that take dense masks")

    def __repr__(self):
        return "RleMasks(M=%d, H=%d, W=%d, runs=%d)" % (self.shape + (len(self.runs),))
