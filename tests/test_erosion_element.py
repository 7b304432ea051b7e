"""The k x k MORPH_ELLIPSE element and its erosion as tests/erosion_ref.py restates them (the reference of the GPU tests in
tests/test_gpu_erosion_element.py), pinned by construction: cv2 is absent, so the element is checked against the matrices OpenCV's
documentation prints and the half-width table of include/lpf.h, the erosion against the oracle's 3x3 cross and hand-made answers.
And the Python layer's validation of ``erosion_kernel_size``, which needs no GPU."""
import numpy as np
import pytest

import erosion_ref as R
from oracle import cpu_oracle as orc


def _rows(*rows):
    return np.array([[int(ch) for ch in row] for row in rows], np.uint8)


def test_element_3_is_the_cross():
    assert np.array_equal(R.ellipse_element(3), _rows("010", "111", "010"))
    assert np.array_equal(R.ellipse_element(1), _rows("1"))


def test_elements_5_and_7_are_the_documented_matrices():
    assert np.array_equal(R.ellipse_element(5), _rows("00100", "11111", "11111", "11111", "00100"))
    assert np.array_equal(R.ellipse_element(7), _rows("0001000", "0111110", "1111111", "1111111", "1111111", "0111110", "0001000"))


TABLE = {3: "0 1 0", 5: "0 2 2 2 0", 7: "0 2 3 3 3 2 0", 9: "0 3 3 4 4 4 3 3 0", 11: "0 3 4 5 5 5 5 5 4 3 0",
         13: "0 3 4 5 6 6 6 6 6 5 4 3 0", 15: "0 4 5 6 6 7 7 7 7 7 6 6 5 4 0"}


@pytest.mark.parametrize("k", sorted(TABLE))
def test_half_widths_match_the_table(k):
    want = [int(t) for t in TABLE[k].split()]
    assert R.half_widths(k) == want
    e = R.ellipse_element(k)
    assert e.shape == (k, k) and e.sum(axis=1).tolist() == [2 * d + 1 for d in want]
    assert np.array_equal(e, e[::-1]) and np.array_equal(e, e[:, ::-1])
    # the table does not depend on the rounding rule: no quotient lies within 0.02 of a tie
    r = k // 2
    for i in range(k):
        q = r * np.sqrt((r * r - (i - r) ** 2) * (1.0 / (r * r)))
        assert abs(q - np.floor(q) - 0.5) > 0.02, (k, i, q)


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (17, 33), (64, 96)])
@pytest.mark.parametrize("iters", [0, 1, 2, 3])
def test_erode_3_is_the_oracles_cross(shape, iters):
    a = (np.random.default_rng(shape[0] * 100 + shape[1]).random(shape) < 0.8).astype(np.uint8)
    want = a
    for _ in range(iters):
        want = orc.erode_cross3(want)
    assert np.array_equal(R.erode(a, 3, iters), want)


@pytest.mark.parametrize("k", [3, 5, 7, 9, 15])
def test_a_zero_pixel_grows_into_the_reflected_element(k):
    a = np.ones((33, 41), np.uint8)
    a[16, 20] = 0
    r = k // 2
    want = np.ones_like(a)
    want[16 - r:16 + r + 1, 20 - r:20 + r + 1] = 1 - R.ellipse_element(k)[::-1, ::-1]
    assert np.array_equal(R.erode(a, k, 1), want)
    # in a corner only the part of the reflection that exists
    b = np.ones((33, 41), np.uint8)
    b[0, 0] = 0
    want = np.ones_like(b)
    want[:r + 1, :r + 1] = 1 - R.ellipse_element(k)[::-1, ::-1][r:, r:]
    assert np.array_equal(R.erode(b, k, 1), want)


@pytest.mark.parametrize("k", [1, 3, 5, 7, 15])
@pytest.mark.parametrize("iters", [0, 1, 3])
def test_a_full_image_stays_full_and_values_take_the_minimum(k, iters):
    assert np.array_equal(R.erode(np.full((9, 20), 255, np.uint8), k, iters), np.full((9, 20), 255, np.uint8))
    a = np.random.default_rng(k).integers(0, 256, (2, 12, 19), dtype=np.uint8)
    got = R.erode(a, k, 1)
    el = R.ellipse_element(k)
    r = k // 2
    for y, x in [(0, 0), (5, 7), (11, 18), (3, 18)]:
        vals = [a[:, y + i - r, x + j - r] for i in range(k) for j in range(k)
                if el[i, j] and 0 <= y + i - r < 12 and 0 <= x + j - r < 19]
        assert np.array_equal(got[:, y, x], np.min(vals, axis=0))
    if k == 1:
        assert np.array_equal(R.erode(a, 1, 5), a)


def test_an_image_smaller_than_the_element_sees_what_exists():
    a = np.ones((3, 5), np.uint8)
    assert np.array_equal(R.erode(a, 7, 2), a)
    a[1, 2] = 0                                              # rows -1 .. 1 of the 7x7 element reach 3 columns to each side
    assert np.array_equal(R.erode(a, 7, 1), np.zeros((3, 5), np.uint8))
    b = np.ones((3, 5), np.uint8)
    b[0, 0] = 0                                              # row dy = 2 has dx = 2: (2, 3) and (2, 4) are out of reach
    want = np.zeros((3, 5), np.uint8)
    want[0, 4] = want[1, 4] = want[2, 3] = want[2, 4] = 1    # (row dy = 0, 1: dx = 3)
    assert np.array_equal(R.erode(b, 7, 1), want)


@pytest.mark.parametrize("bad", [0, 4, 17, "5", -3, 5.0, True, None])
def test_python_layer_refuses_a_bad_size_before_any_gpu_work(bad):
    from lidar_object_detection_amd import pipeline
    for fn in (pipeline.run_frames, pipeline.car_statistics_v3_frames):
        with pytest.raises(ValueError, match="erosion_kernel_size"):
            fn([], None, None, erosion_kernel_size=bad)
    with pytest.raises(ValueError, match="erosion_kernel_size"):
        pipeline.run_frames_multicam([[]], [(None, None)], erosion_kernel_size=bad)
    with pytest.raises(ValueError, match="erosion_kernel_size"):
        pipeline.process_frames(segmenter=lambda im: None, kitti360_path="/nonexistent", erosion_kernel_size=bad)
    with pytest.raises(ValueError, match="erosion_kernel_size"):
        next(pipeline.stream_frames([], None, None, None, erosion_kernel_size=bad))


def test_default_and_good_sizes_pass_without_frames():
    from lidar_object_detection_amd import pipeline
    assert pipeline.run_frames([], None, None) == []
    for k in (1, 3, 5, 15, np.int64(7)):
        assert pipeline.run_frames([], None, None, erosion_kernel_size=k) == []
    assert "lpf_set_erosion_element" in __import__("lidar_object_detection_amd._native", fromlist=["EXPORTED"]).EXPORTED
