"""seg_with_pointcloud.py:174-180 restated in NumPy, and the inputs of tests/golden/depth_overlays_golden.json
(tests/golden/make_golden_overlays.py): the seeded segmented images and the frames' depth-map lists.

The script, once per car with a nonzero depth map:
    depthImage = cm(depthMap / np.max(depthMap))[..., :3]            # cm = plt.get_cmap('jet')
    image_withseg = np.array(masking_image) / 255.
    image_withseg[depthMap > 0] = depthImage[depthMap > 0]
    image_withseg = np.uint8(image_withseg * 255)
    image_withseg = cv2.cvtColor(image_withseg, cv2.COLOR_RGB2BGR)
Byte for byte: a listed pixel is the reversed LUT[min(255, int(256 * (d / mx)))], any other pixel the reversed segmented pixel."""
import hashlib
import json
import os

import numpy as np

from conftest import GOLDEN, golden_frames, load_golden, unpack_masks

FULL = (1461, 2098, 2449)
DMAX = 30.0
SEG_SEED = 1700000                    # segmented image of a frame: default_rng(SEG_SEED + frame (+ FULL_SEED_OFFSET at full size))
FULL_SEED_OFFSET = 50000


def jet_lut():
    """(cm._lut[:256, :3] * 255).astype(np.uint8) of matplotlib's 'jet', as committed"""
    return np.load(os.path.join(GOLDEN, "jet_lut_u8.npy"))


def load_overlay_golden():
    with open(os.path.join(GOLDEN, "depth_overlays_golden.json")) as f:
        return json.load(f)


def seg_image(frame, full, H, W):
    """the seeded stand-in for the segmenter's image of a frame: uint8 [H,W,3]"""
    rng = np.random.default_rng(SEG_SEED + frame + (FULL_SEED_OFFSET if full else 0))
    return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


def overlay(seg, pix, depth, lut=None):
    """(image uint8 [H,W,3], mx) of one car: the script's statements on a sparse list (pix ascending flat v * W + u, depth > 0)"""
    lut = jet_lut() if lut is None else lut
    img = np.ascontiguousarray(seg[..., ::-1])
    mx = float(np.max(depth)) if len(depth) else 0.0
    if len(pix):
        i = np.minimum(255, (256.0 * (np.asarray(depth, np.float64) / mx)).astype(np.int64))
        img.reshape(-1, 3)[pix] = lut[i][:, ::-1]
    return img, mx


def sha(img):
    return hashlib.sha256(np.ascontiguousarray(img, np.uint8).tobytes()).hexdigest()


def golden_inputs(H, W):
    """key -> dict(frame, full, pts f32 [N,4], rect5 / edge uint8 [M,H,W], seg uint8 [H,W,3]) for the 20 sample frames (key =
    frame) and the 3 full-size ones (key = "full_<frame>"), in the order of the golden JSON"""
    out = {}
    for r in golden_frames()["frames"]:
        f = r["frame"]
        g = load_golden(f)
        d = dict(frame=f, full=False, pts=np.ascontiguousarray(g["points"], np.float32), seg=seg_image(f, False, H, W))
        for kind in ("rect5", "edge"):
            key = "masks_%s_packed" % kind
            d[kind] = unpack_masks(g, kind, H, W).astype(np.uint8) if key in g else np.zeros((0, H, W), np.uint8)
        out[str(f)] = d
    for f in FULL:
        g = dict(np.load(os.path.join(GOLDEN, "frame_%010d_full.npz" % f)))
        out["full_%d" % f] = dict(frame=f, full=True, pts=np.ascontiguousarray(g["points"], np.float32), seg=seg_image(f, True, H, W),
                                  rect5=unpack_masks(g, "rect5", H, W).astype(np.uint8), edge=unpack_masks(g, "edge", H, W).astype(np.uint8))
    return out
