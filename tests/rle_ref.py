"""Run-length masks restated in plain NumPy loops, independent of lidar_object_detection_amd/rle.py (it imports nothing from it): the
yardstick of the RleMasks tests.  A run (start, length) is the pixels start .. start + length - 1 of the image flattened row-major; a
pixel is a member iff any run of its mask holds it.  Slow on purpose: one pixel, one run at a time."""
import numpy as np


def dense_to_runs(mask2d):
    """Canonical runs [(start, length)] of one [H,W] mask (member = nonzero): ascending, maximal."""
    flat = np.asarray(mask2d).reshape(-1) != 0
    runs, start = [], None
    for p, v in enumerate(flat.tolist()):
        if v and start is None:
            start = p
        elif not v and start is not None:
            runs.append((start, p - start))
            start = None
    if start is not None:
        runs.append((start, len(flat) - start))
    return runs


def dense_to_runs_fast(mask2d):
    """The same runs for large images (1408 x 376): boundaries from one shifted comparison."""
    flat = np.asarray(mask2d).reshape(-1) != 0
    prev = np.concatenate(([False], flat[:-1]))
    nxt = np.concatenate((flat[1:], [False]))
    starts = np.flatnonzero(flat & ~prev)
    ends = np.flatnonzero(flat & ~nxt)
    return [(int(s), int(e - s + 1)) for s, e in zip(starts, ends)]


def runs_to_dense(runs, H, W):
    """uint8 [H,W] of any list of runs (any order, overlaps allowed)."""
    flat = np.zeros(H * W, np.uint8)
    for start, length in runs:
        assert 0 <= start and 0 <= length and start + length <= H * W
        flat[start:start + length] = 1
    return flat.reshape(H, W)


def masks_to_dense(runs, run_off, M, H, W):
    """uint8 [M,H,W] of a runs / run_off pair."""
    runs = np.asarray(runs).reshape(-1, 2)
    return np.stack([runs_to_dense([tuple(int(v) for v in r) for r in runs[int(run_off[m]):int(run_off[m + 1])]], H, W)
                     for m in range(M)]) if M else np.zeros((0, H, W), np.uint8)


def coco_counts_to_dense(counts, H, W):
    """COCO's uncompressed counts -> uint8 [H,W]: column-major, alternating zeros / ones, zeros first."""
    col = []
    value = 0
    for c in counts:
        col += [value] * int(c)
        value ^= 1
    assert len(col) == H * W
    out = np.zeros((H, W), np.uint8)
    for k, v in enumerate(col):
        out[k % H, k // H] = v
    return out


def dense_to_coco_counts(mask2d):
    """uint8 [H,W] -> COCO's uncompressed counts."""
    col = (np.asarray(mask2d) != 0).T.reshape(-1).tolist()
    counts, value, n = [], False, 0
    for v in col:
        if v == value:
            n += 1
        else:
            counts.append(n)
            value, n = v, 1
    counts.append(n)
    return counts
