"""NumPy restatement of the k x k MORPH_ELLIPSE erosion (include/lpf.h: lpf_set_erosion_element), the reference of
tests/test_erosion_element.py and tests/test_gpu_erosion_element.py.  cv2 is absent, so -- like the 3x3 erosion
and the resize -- the element is pinned by construction: OpenCV's getStructuringElement(MORPH_ELLIPSE, (k, k)) for odd k is, with
r = k // 2, row i (dy = i - r) = ones from column r - dx to r + dx inclusive, dx = round_half_even(r * sqrt((r*r - dy*dy) / (r*r)))."""
import numpy as np


def half_widths(k):
    """dx of each of the k rows of the element."""
    if k < 1 or k % 2 == 0:
        raise ValueError("odd k >= 1, got %r" % (k,))
    r = k // 2
    if r == 0:
        return [0]
    inv_r2 = 1.0 / (r * r)
    return [int(np.rint(r * np.sqrt((r * r - (i - r) * (i - r)) * inv_r2))) for i in range(k)]      # (np.rint rounds half to even)


def ellipse_element(k):
    """uint8 [k, k]: cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (k, k)) for odd k."""
    r = k // 2
    e = np.zeros((k, k), np.uint8)
    for i, dx in enumerate(half_widths(k)):
        e[i, r - dx:r + dx + 1] = 1
    return e


def erode(a, k, iters=1):
    """cv2.erode(a, ellipse_element(k), iterations=iters) on the last two axes of ``a`` (any leading axes; uint8 values or 0 / 1
    members): the minimum over the element's pixels, pixels outside the image left out (the border is +infinity).  Several iterations
    repeat one iteration."""
    a = np.asarray(a)
    r = k // 2
    el = ellipse_element(k)
    top = np.iinfo(a.dtype).max if a.dtype.kind in "ui" else np.inf
    H, W = a.shape[-2:]
    for _ in range(iters):
        p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(r, r), (r, r)], constant_values=top)
        out = np.full_like(a, top)
        for i in range(k):
            for j in range(k):
                if el[i, j]:
                    out = np.minimum(out, p[..., i:i + H, j:j + W])
        a = out
    return a
