"""Same_color.py:113-132, the exclusive first-mask-wins labelling, restated in NumPy (TEST ONLY): what lpf_first_match,
LpfContext.first_match and pipeline.first_match_frames are compared with.  The script walks the valid points in ascending order and
gives each to the first mask of its list with ``y < mask.shape[0] and x < mask.shape[1] and mask[y, x] > 0.5``; here the same test
runs mask by mask over the points no earlier mask took.  tests/test_first_match_api.py pins it against what the script's own lines
produced (tests/golden/first_match_golden.npz, made by tests/golden/make_golden_first_match.py), on the committed frames and on the
constructed cases below, which the generator and the tests both regenerate from their seeds."""
import numpy as np

from oracle import numpy_path as NP

DMAX = 30.0                                 # the script's depth window is (0, 30)


def project(points, T, K3, W, H, dmax=DMAX):
    """Same_color.py:93-96 + :114: (u, v, valid) of points f32 [N,4] (the statements of oracle.numpy_path.frame_path)"""
    points_homo = points.copy()
    points_homo[:, 3] = 1
    pointsCam = np.matmul(T, points_homo.T).T[:, :3]
    u, v, depth = NP.cam2image(K3, pointsCam.T)
    valid = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (depth > 0) & (depth < dmax)
    return u, v, valid


def first_match(u, v, valid, masks, colors=None):
    """The loop of Same_color.py:120-132 over the points where ``valid``: masks is the script's list (each mask at its OWN size),
    colors its mask_colors.  Returns first_mask int32 [N] (-2 not valid, -1 valid and in no mask, else the first mask), car_idx /
    car_mask / bg_idx in ascending point order, mask_count int64 [M] and, with colors, car_rgb = np.array(mask_colors[i]) / 255.0."""
    u, v, valid = np.asarray(u), np.asarray(v), np.asarray(valid, bool)
    code = np.where(valid, -1, -2).astype(np.int32)
    pending = valid.copy()
    for m, mask in enumerate(masks):
        mask = np.asarray(mask)
        idx = np.flatnonzero(pending & (v < mask.shape[0]) & (u < mask.shape[1]))
        with np.errstate(invalid="ignore"):
            hit = idx[mask[v[idx], u[idx]] > 0.5]
        code[hit] = m
        pending[hit] = False
    car = np.flatnonzero(code >= 0).astype(np.int64)
    out = {"first_mask": code, "car_idx": car, "car_mask": code[car], "bg_idx": np.flatnonzero(code == -1).astype(np.int64),
           "mask_count": np.bincount(code[car], minlength=len(masks)).astype(np.int64)}
    if colors is not None:
        table = np.array([np.array(c) / 255.0 for c in colors], np.float64).reshape(-1, 3)
        out["car_rgb"] = table[code[car]]
    return out


# ---- constructed cases, regenerated from seeds ---------------------------------------------------------------------------------------
FLOAT_VALUES = (np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(1)), np.float32(np.nan), np.float32(-1.0), np.float32(np.inf),
                np.float32(1e-45))                          # (1e-45 rounds to the smallest float32 subnormal, 2^-149)
FLOAT_MEMBER = (False, True, False, False, True, False)     # which of them are > 0.5
CASES = ("overlap_f32", "overlap_u8", "small", "large", "values", "no_mask", "no_valid")


def points_at(pix, depth, T, K3):
    """float32 [n,4] velodyne points that project to the pixel centres pix [n,2] = (u, v) at the given depths (float64 [n])"""
    pix, depth = np.asarray(pix, np.float64).reshape(-1, 2), np.asarray(depth, np.float64).reshape(-1)
    cam = np.linalg.solve(K3, np.vstack([pix[:, 0] * depth, pix[:, 1] * depth, depth]))
    velo = np.linalg.solve(T, np.vstack([cam, np.ones(len(depth))]))
    out = np.ones((len(depth), 4), np.float32)
    out[:, :3] = velo[:3].T
    return out


def _scatter(rng, n, W, H, T, K3):
    """n points over (and a little beyond) the image, a few too far, a few behind the camera"""
    pix = np.stack([rng.integers(-20, W + 20, n), rng.integers(-10, H + 10, n)], axis=1)
    depth = rng.uniform(2.0, 29.0, n)
    depth[rng.random(n) < 0.1] = rng.uniform(31.0, 60.0)
    depth[rng.random(n) < 0.05] = -5.0
    return points_at(pix, depth, T, K3)


def _rects(rng, M, mh, mw, dtype):
    masks = np.zeros((M, mh, mw), dtype)
    for m in range(M):
        x0, y0 = int(rng.integers(0, mw * 3 // 4)), int(rng.integers(0, mh * 3 // 4))
        w, h = int(rng.integers(mw // 8, mw // 2)), int(rng.integers(mh // 8, mh // 2))
        masks[m, y0:y0 + h, x0:x0 + w] = rng.integers(1, 255) if dtype == np.uint8 else 1.0
    return masks


def constructed_case(name, calib):
    """(points f32 [N,4], masks: the script's list of [mh,mw] arrays) of one of CASES, from the camera of the committed calibration"""
    T, K3, W, H = calib["TrVeloToRect"], calib["K"][:3, :3], int(calib["width"]), int(calib["height"])
    rng = np.random.default_rng(1000 + CASES.index(name))
    if name in ("overlap_f32", "overlap_u8"):
        dtype = np.float32 if name == "overlap_f32" else np.uint8
        masks = _rects(rng, 6, H, W, dtype)
        masks[0, 100:200, 300:700] = 1                      # three masks over one region: first != last there
        masks[2, 150:250, 500:900] = 1
        masks[4, 120:220, 600:800] = 1
        masks[:5, 300:, 1200:] = 0                          # a corner only the last mask covers
        masks[5, 300:, 1200:] = 1
        pts = np.concatenate([_scatter(rng, 1500, W, H, T, K3),
                              points_at([[650, 160], [1300, 340], [1407, 375]], [10.0, 12.0, 8.0], T, K3)])
        return pts, list(masks)
    if name in ("small", "large"):
        mh, mw = (H - 100, W - 300) if name == "small" else (H + 5, W + 7)
        masks = _rects(rng, 3, mh, mw, np.float32)
        masks[2] = 1.0                                      # the last mask takes everything inside its own size
        eu, ev = min(mw, W - 1), min(mh, H - 1)
        edge = [[mw - 1, 50], [eu, 50], [60, mh - 1], [60, ev], [mw - 1, mh - 1], [eu, ev], [W - 1, H - 1], [0, 0]]
        pts = np.concatenate([_scatter(rng, 800, W, H, T, K3), points_at(edge, np.full(len(edge), 9.0), T, K3)])
        return pts, list(masks)
    if name == "values":
        masks = np.zeros((2, H, W), np.float32)
        masks[1] = 1.0
        pix = [[100 + 10 * i, 200] for i in range(len(FLOAT_VALUES))]
        for (x, y), val in zip(pix, FLOAT_VALUES):
            masks[0, y, x] = val
        return np.concatenate([points_at(pix, np.full(len(pix), 7.0), T, K3), _scatter(rng, 200, W, H, T, K3)]), list(masks)
    if name == "no_mask":
        return _scatter(rng, 500, W, H, T, K3), []
    if name == "no_valid":
        pix = np.stack([rng.integers(0, W, 300), rng.integers(0, H, 300)], axis=1)
        return points_at(pix, np.where(rng.random(300) < 0.5, -3.0, 45.0), T, K3), list(_rects(rng, 2, H, W, np.float32))
    raise KeyError(name)


def golden_frame_case(g, calib):
    """(points, the script's mask list) of a committed frame: its overlapping "edge" masks (a frame without them: its "rect5" masks,
    or none), float32 0 / 1 at the camera's size"""
    W = int(calib["width"])
    for kind in ("edge", "rect5"):
        if "masks_%s_packed" % kind in g:
            return g["points"], list(np.unpackbits(g["masks_%s_packed" % kind], axis=-1)[..., :W].astype(np.float32))
    return g["points"], []
