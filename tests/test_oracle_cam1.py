"""Camera 1 of the sample rig, pinned: the C oracle (oracle/lpf_oracle.c) and the NumPy path (oracle/numpy_path.py) against the
camera-1 golden vectors of tests/golden/make_golden_cam1.py -- the reference's own V3:524-535 with cam_id = 1, its camera-1 box
handling (the cam-0 corners through camera 1's TrVeloToCam, the visibility filter with camera 1) and its projection, clip, masks,
box counts and statistics."""
import os

import numpy as np
import pytest

from cam1_fixtures import cam1_frames, load_calib1, load_cam1_golden
from conftest import GOLDEN, unpack_masks
from oracle import cpu_oracle as orc
from oracle import numpy_path as npp

CAM1 = cam1_frames()
_cam1 = load_cam1_golden


@pytest.fixture(scope="module")
def calib1():
    return load_calib1()


def test_camera1_calibration_is_its_own(calib, calib1):
    assert CAM1["cam_id"] == 1 and {r["frame"] for r in CAM1["frames"]} >= {100, 2449}
    assert not np.array_equal(calib1["TrVeloToRect"], calib["TrVeloToRect"])
    assert np.allclose(calib1["TrVeloToRect"], calib1["R_rect_01"] @ calib1["TrVeloToCam"], rtol=0, atol=0)
    assert int(calib1["width"]) == int(calib["width"]) and int(calib1["height"]) == int(calib["height"])
    assert "P_rect_01" in str(calib1["perspective_txt"]) and "image_01" in str(calib1["calib_cam_to_pose_txt"])


@pytest.mark.parametrize("rec", CAM1["frames"], ids=lambda r: "f%d" % r["frame"])
def test_oracle_reproduces_camera1(rec, calib1):
    g = _cam1(rec["frame"])
    T, K = calib1["TrVeloToRect"], calib1["K"][:, :3]
    W, H = int(calib1["width"]), int(calib1["height"])
    o = orc.project(g["points"], T, K)
    assert np.array_equal(o["u64"], g["u"]) and np.array_equal(o["v64"], g["v"])
    masks = unpack_masks(g, "rect5", H, W)
    M = masks.shape[0]
    r = orc.run(g["points"], T, K, W, H, 0.0, 50.0, label_img=orc.pack_masks(orc.binarize_f32(masks, 0), 0, H, W), M=M,
                corners=g["corners_velo"], oriented=True)
    assert np.array_equal(r["valid_idx"], g["valid_idx_d50"])
    assert np.array_equal(r["inst_count"], g["inst_count_rect5_d50"])
    assert np.array_equal(np.concatenate(r["inst_lists"]) if M else np.zeros(0, np.int64), g["inst_cat_rect5_d50"])
    assert np.array_equal(r["count_mb"], g["count_mb_rect5_d50"])
    rows = [m for m in range(M) if r["inst_count"][m] > 0] if len(g["corners_velo"]) else []
    assert np.array_equal(np.array(rows, np.int64), g["stats_car_id_rect5_d50"])
    assert np.array_equal(np.array([r["best_box"][m] if r["best_cnt"][m] >= 10 else -1 for m in rows], np.int64),
                          g["stats_matched_bbox_id_rect5_d50"])
    assert np.array_equal(np.array([r["best_cnt"][m] if r["best_cnt"][m] >= 10 else 0 for m in rows], np.int64),
                          g["stats_points_inside_bbox_rect5_d50"])
    assert np.array_equal(r["inst_count"][rows], g["stats_total_points_rect5_d50"])


@pytest.mark.parametrize("rec", CAM1["frames"], ids=lambda r: "f%d" % r["frame"])
def test_numpy_path_reproduces_camera1(rec, calib1):
    g = _cam1(rec["frame"])
    W, H = int(calib1["width"]), int(calib1["height"])
    masks = unpack_masks(g, "rect5", H, W)
    u, v, vi, lists, cnt, bb, bc = npp.frame_path(g["points"], calib1["TrVeloToRect"], calib1["K"][:, :3], W, H, 50.0, masks,
                                                  g["corners_velo"])
    assert np.array_equal(u, g["u"]) and np.array_equal(v, g["v"]) and np.array_equal(vi, g["valid_idx_d50"])
    assert np.array_equal(np.concatenate(lists) if lists else np.zeros(0, np.int64), g["inst_cat_rect5_d50"])
    assert np.array_equal(cnt, g["count_mb_rect5_d50"])


def test_camera1_boxes_are_the_reference_quirk(calib, calib1):
    """Frame 2449: the cam-0 corners placed with camera 1's TrVeloToCam (the camera-to-camera offset) -- not camera 0's corners."""
    g1, g0 = _cam1(2449), dict(np.load(os.path.join(GOLDEN, "frame_0000002449.npz")))
    assert np.array_equal(g1["corners_cam0_raw"], g0["corners_cam0_raw"])
    pos = g1["visible_pos"]
    c = g1["corners_cam0_raw"][pos]
    hom = np.concatenate([c, np.ones(c.shape[:2] + (1,))], axis=2)
    velo = np.einsum("ij,bkj->bki", np.linalg.inv(calib1["TrVeloToCam"]), hom)[..., :3]
    assert np.allclose(velo, g1["corners_velo"], atol=1e-9)
    assert not np.array_equal(g1["visible_pos"], g0["visible_pos"]) or not np.allclose(g1["corners_velo"], g0["corners_velo"])
