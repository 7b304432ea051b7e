"""Camera 1 of the sample rig (tests/golden/make_golden_cam1.py): its calibration and golden vectors.  A camera-1 file does not hold
the scan again: the scan is camera 0's golden scan of the same frame, and the file holds its SHA-256, checked here."""
import hashlib
import json
import os

import numpy as np

from conftest import GOLDEN, load_golden


def load_calib1():
    return dict(np.load(os.path.join(GOLDEN, "calib_cam1.npz")))


def cam1_frames():
    with open(os.path.join(GOLDEN, "cam1_index.json")) as f:
        return json.load(f)


def load_cam1_golden(frame):
    g = dict(np.load(os.path.join(GOLDEN, "cam1_frame_%010d.npz" % frame)))
    pts = load_golden(frame)["points"]
    if hashlib.sha256(np.ascontiguousarray(pts).tobytes()).digest() != g["points_sha256"].tobytes():
        raise AssertionError("camera 0's golden scan of frame %d is not the scan camera 1's golden vectors were made from" % frame)
    g["points"] = pts
    return g
