"""Case generator and checker of the seeded differential fuzz of the wide and multi-camera passes (lpf_run_wide, lpf_run_frame_wide,
lpf_run_cams, lpf_run_cams_wide, lpf_depth_maps): tests/test_gpu_fuzz_wide.py runs the cases on the GPU, tests/test_wide_fuzz_cases.py
proves on the CPU, from the oracle alone, that the default seeds reach the edges they are meant to reach and that the checker notices
a single wrong entry.  Not a test module.

case(seed, calib) is deterministic from the seed alone.  Values whose presence the CPU test asserts are partly laid out by the seed
itself (the empty-frame layout by the seed modulo 14; mask count, image size, mask kind, the first frame's box count and the sizes of
two frames by the seed's rank among the cases with points, modulo the length of each list), the rest is drawn from default_rng(seed).

Every camera is the sample camera resampled to another sensor size (K scaled as tests/test_gpu_mask_rects.py scales it), so a point
keeps its place in the image, relative to the image's size, in every camera.  The clouds come from test_gpu_fuzz._frustum_cloud at
the 1408 x 376 size: its margins of 40 and 20 pixels there are the same fraction of every other size."""
import os

import numpy as np

from lidar_object_detection_amd import synthetic as S
from lidar_object_detection_amd._native import LpfContext
from oracle import cpu_oracle as orc
from test_gpu_fuzz import _frustum_cloud
from test_gpu_mask_rects import _outside_zeroed
from test_gpu_wide_masks import _check

DEFAULT_CASES = 14                                    # every layout once or more, and 12 cases with points: see rank
DEFAULT_SEED_BASE = 3027                              # a base whose 14 seeds meet tests/test_wide_fuzz_cases.py: about a third of all do

CAMERAS = [(1408, 376), (1242, 375), (150, 37), (17, 16), (70, 33)]
SIZES = [0, 1, 3, 4, 5, 63, 1023, 1024, 1025, 2049, 4097, 9000, 20000]
MASK_COUNTS = [0, 1, 31, 32, 33, 48, 49, 64, 65, 100, 255, 256]
BOX_COUNTS = [0, 1, 7, 64, 65, 130]
SIZE_WEIGHTS = np.array([1.0] * 11 + [2.0, 3.0]) / 16.0     # the drawn sizes lean to the large frames: dense lists need them
INSIDE = [0.0, 0.3, 0.9]
INSIDE_WEIGHTS = [0.2, 0.3, 0.5]
DEPTH_MAX = [30.0, 50.0, 80.0]
ODD = np.array([0.5, 0.50000006, 0.999, 1.5, 256.0, np.nan, -1.0], np.float32)
RULES = ["astype", "v3", "gt0.5"]                     # orc.binarize_f32's codes 0, 1, 2
KINDS = ["astype", "v3", "gt0.5", "u8", "astype", "v3", "gt0.5"]      # by the seed: float32 masks under a rule, or uint8 masks
LAYOUTS = ["drawn", "all", "first", "drawn", "last", "drawn", "two", "drawn", "single", "drawn", "first", "last", "two", "drawn"]
FULL, RANDOM, RECT, EMPTY, DISK = range(5)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
MASK_BYTES = 140 << 20                                # masks of one camera of one case, as uint8: frames are dropped beyond it
FLOAT_ELEMS = 48 << 20                                # float32 masks only below this many mask pixels
LADDER_SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 0, 0, 4097, 262145, 0]


def default_seeds():
    """the seeds of a run without LPF_FUZZ_CASES / LPF_FUZZ_SEED_BASE: the ones the CPU test asserts its conditions over"""
    return [DEFAULT_SEED_BASE + i for i in range(DEFAULT_CASES)]


def seeds():
    """the seeds of this run (LPF_FUZZ_CASES, LPF_FUZZ_SEED_BASE as tests/test_gpu_fuzz.py reads them)"""
    base = int(os.environ.get("LPF_FUZZ_SEED_BASE", str(DEFAULT_SEED_BASE)))
    return [base + i for i in range(int(os.environ.get("LPF_FUZZ_CASES", str(DEFAULT_CASES))))]


def scaled_K(K0, W0, H0, W, H):
    K = np.array(K0, dtype=np.float64)[:3, :3].copy()
    K[0, 0] *= W / W0; K[0, 2] *= W / W0; K[1, 1] *= H / H0; K[1, 2] *= H / H0           # the same field of view on the other sensor
    return K


def empty_layouts(sizes):
    """which of the five empty-frame layouts a batch of these frame sizes is"""
    z = [n == 0 for n in sizes]
    out = set()
    if len(z) == 1:
        return {"single"} if z[0] else out
    if all(z):
        return {"all"}
    if z[0]:
        out.add("first")
    if z[-1]:
        out.add("last")
    if any(a and b for a, b in zip(z, z[1:])):
        out.add("two")
    return out


def rank(seed):
    """The seed's place among the seeds whose layout has points (every 14 seeds hold one "all" and one "single" case, which show
    nothing of a mask count or a frame size): the mask count, the image size and the two laid-out frame sizes go by it, so 14
    consecutive seeds put each of the 12 mask counts on frames with points."""
    n, r = divmod(seed, len(LAYOUTS))
    return seed - 2 * n - (r > LAYOUTS.index("all")) - (r > LAYOUTS.index("single"))


def _frame_sizes(seed, rng):
    """(points per frame, the empty-frame layout, the frame made dense or None, ``lead`` or None).  Two frames take their size from the seed's rank r,
    SIZES[r % 13] in slot ``lead`` (frame 0; frame 1 under "first") and SIZES[(r + 4) % 13] behind it, where no layout takes them
    away: the 12 ranks of 14 consecutive seeds lay out 12 sizes in the first slot and the thirteenth in the second.  The cases of 65
    and of 255 masks get a 20 000-point frame with 90 % inside behind these: the dense lists."""
    layout = LAYOUTS[seed % len(LAYOUTS)]
    F = int(rng.integers(1, 6))
    sizes = [int(rng.choice(SIZES, p=SIZE_WEIGHTS)) for _ in range(5)]
    if layout == "single":
        return [0], layout, None, None
    if layout == "all":
        return [0] * max(F, 2), layout, None, None
    lead = 1 if layout == "first" else 0
    r = rank(seed)
    dense = lead + 2 if MASK_COUNTS[r % len(MASK_COUNTS)] in (65, 255) else None
    head = lead + 2 + (dense is not None)                     # the frames the layout leaves alone
    F = min(5, max(F, head + {"drawn": 0, "first": 0, "last": 1, "two": 2}[layout]))
    sizes = [n or 1025 for n in sizes[:F]]                    # (zeros come from the layout, or from the seed's own sizes)
    sizes[lead], sizes[lead + 1] = SIZES[r % len(SIZES)], SIZES[(r + 4) % len(SIZES)]
    if dense is not None:
        sizes[dense] = 20000
    if layout == "first":
        sizes[0] = 0
    elif layout == "last":
        sizes[-1] = 0
    elif layout == "two":
        at = int(rng.integers(head, F - 1))
        sizes[at] = sizes[at + 1] = 0
    elif rng.random() < 0.3 and F > head:
        sizes[int(rng.integers(head, F))] = 0                 # "drawn": now and then an empty frame somewhere
    return sizes, layout, dense, lead


def _draw_masks(rng, F, M, W, H):
    """uint8 [F,M,H,W]: per mask full, random 0.5, a rectangle, empty or a disk; with more than 32 masks the last label word of every
    frame holds at least one full or random mask.  A third of the frames have no full mask and one random mask at the most (the
    others become rectangles and disks): their masked points are a proper part of their valid points, whatever M is."""
    m = np.zeros((F, M, H, W), np.uint8)
    kinds = rng.integers(0, 5, size=(F, M))
    first_of_last = 32 * ((M + 31) // 32 - 1)
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    for f in range(F):
        if rng.random() < 0.34:
            kinds[f] = np.where(kinds[f] == FULL, RECT, np.where(kinds[f] == RANDOM, DISK, kinds[f]))
            if M > 32:
                kinds[f, int(rng.integers(first_of_last, M))] = RANDOM
        elif M > 32 and not np.isin(kinds[f, first_of_last:], (FULL, RANDOM)).any():
            kinds[f, int(rng.integers(first_of_last, M))] = int(rng.choice([FULL, RANDOM]))
        for i in range(M):
            k = kinds[f, i]
            if k == FULL:
                m[f, i] = 1
            elif k == RANDOM:
                m[f, i] = rng.integers(0, 2, size=(H, W), dtype=np.uint8)
            elif k == RECT:
                x0, y0 = int(rng.integers(0, W)), int(rng.integers(0, H))
                m[f, i, y0:y0 + int(rng.integers(1, max(2, H // 2))), x0:x0 + int(rng.integers(1, max(2, W // 2)))] = 1
            elif k == DISK:
                r = rng.uniform(0.06, 0.33) * max(H, 12)
                cx, cy = rng.uniform(0, W), rng.uniform(0, H)
                m[f, i] = (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
    return m


def _with_sentinels(rng, rects):
    """some coordinates replaced by "no limit": a looser rectangle still holds"""
    r = rects.astype(np.int64)
    pick = rng.random(r.shape) < 0.3
    lim = np.broadcast_to(np.array([I32_MIN, I32_MIN, I32_MAX, I32_MAX], np.int64), r.shape)
    return np.where(pick, lim, r).astype(np.int32)


def _rects_that_do_not_hold(rng, F, M, W, H):
    """random rectangles, some of them beyond the image, empty or inverted: the masks have bytes outside them"""
    r = np.zeros((F, M, 4), np.int32)
    for f in range(F):
        for m in range(M):
            x0, y0 = int(rng.integers(-5, W)), int(rng.integers(-5, H))
            r[f, m] = (x0, y0, int(rng.integers(x0, W + 6)), int(rng.integers(y0, H + 6)))
        if M:
            r[f, 0] = (I32_MIN, 1, W - 1, I32_MAX)
        if M > 1:
            r[f, 1] = (3, 2, 2, 9)                                                  # inverted
    return r


def clipped(rects, W, H):
    c = rects.astype(np.int64)
    c[..., 0] = np.clip(c[..., 0], 0, W); c[..., 2] = np.clip(c[..., 2], 0, W)
    c[..., 1] = np.clip(c[..., 1], 0, H); c[..., 3] = np.clip(c[..., 3], 0, H)
    return c


def zeroed_outside(cam, which, f):
    """frame f's binarised masks zeroed outside lpf_run_frame_wide's rectangles ``which``, clipped to the image"""
    rects = clipped(cam["fw_rects"][which][f], cam["W"], cam["H"])
    return _outside_zeroed(cam["member"][f][None], rects[None])[0]


def _draw_boxes(rng, B):
    """B boxes in the frustum, half of them scaled up about their centres (counts well above one), and, for two boxes or more, often
    the last one a copy of the first: equal counts, which the first strict maximum has to resolve"""
    if B == 0:
        return np.zeros((0, 8, 3))
    cor = S.synthetic_boxes(B, seed=int(rng.integers(1 << 30)))[1].copy()
    scale = rng.choice([1.0, 1.0, 3.0, 6.0], size=B)
    centre = cor.mean(axis=1, keepdims=True)
    cor = centre + (cor - centre) * scale[:, None, None]
    if B >= 2 and rng.random() < 0.7:
        cor[B - 1] = cor[0]
    return np.ascontiguousarray(cor)


def camera_shape(index, n_frames, max_masks, size=None, M=None):
    """(W, H, M, F) of the camera that ``index`` lays out over n_frames frames: F frames of masks fit the byte budget"""
    W, H = size or CAMERAS[index % len(CAMERAS)]
    counts = [m for m in MASK_COUNTS if m <= max_masks]
    if M is None:                                             # (the short list of run_cams shifts with every turn: not tied to seed % 4)
        M = counts[(index + (index // len(counts) if max_masks < 256 else 0)) % len(counts)]
    F = n_frames
    while F > 1 and F * M * H * W > MASK_BYTES:               # (the frames beyond F keep their points; this camera's case ends at F)
        F -= 1
    return W, H, M, F


def case_shapes(seed, n_cams, max_masks=256):
    """(points per frame, [(W, H, M, F) per camera]) of case(seed, ...), without drawing anything else"""
    sizes = _frame_sizes(seed, np.random.default_rng(seed))[0]
    return sizes, [camera_shape(rank(seed) + 7 * k, len(sizes), max_masks) for k in range(n_cams)]


def _draw_camera(index, rng, calib, sizes, max_masks, size=None, M=None):
    """One camera of a case over frames of ``sizes`` points: image size, depth window, masks, boxes, rectangles.  index lays out the
    values the CPU test counts (see the module docstring)."""
    _, T, K0, W0, H0 = S.default_calibration(calib)
    W, H, M, F = camera_shape(index, len(sizes), max_masks, size, M)
    cam = dict(T=np.asarray(T, np.float64), K=scaled_K(K0, W0, H0, W, H), W=W, H=H, dmin=0.0, dmax=float(rng.choice(DEPTH_MAX)), M=M, F=F,
               oriented=bool(rng.integers(0, 2)), erode=int(rng.choice([0, 0, 1, 2])))
    u8 = _draw_masks(rng, F, M, W, H)
    kind = KINDS[index % len(KINDS)]
    cam["kind"] = "f32" if (kind != "u8" and F * M * H * W <= FLOAT_ELEMS) else "u8"
    cam["binarize"] = kind if cam["kind"] == "f32" else "astype"
    if cam["kind"] == "f32":
        fm = u8.astype(np.float32)
        for f in range(F):
            if M:                                             # (in the first word: the forced mask of the last word stays as it is)
                fm[f, int(rng.integers(0, min(M, 32)))] *= rng.choice(ODD, size=(H, W))
        cam["masks"] = fm
        cam["member"] = orc.binarize_f32(fm, RULES.index(cam["binarize"]))
    else:
        cam["masks"] = u8 * np.uint8(rng.choice([1, 200, 255]))
        cam["member"] = u8
    B0 = BOX_COUNTS[index % len(BOX_COUNTS)]
    cam["boxes"] = [_draw_boxes(rng, B0 if f == 0 else int(rng.choice(BOX_COUNTS))) for f in range(F)]
    mode = ["none", "tight", "sentinel"][int(rng.integers(0, 3))]
    if cam["erode"] or M == 0:                                # rectangles describe the masks as given: not what erosion leaves
        mode = "none"
    tight = LpfContext.mask_rects(cam["member"]) if M else np.zeros((F, 0, 4), np.int32)
    cam["rects_mode"] = mode
    cam["rects"] = None if mode == "none" else tight if mode == "tight" else _with_sentinels(rng, tight)
    # lpf_run_frame_wide's own rectangles (uint8 masks = member, no erosion): ones that hold (tight, or with sentinels) and ones that
    # do not
    cam["fw_mode"] = ["tight", "sentinel"][int(rng.integers(0, 2))]
    cam["fw_rects"] = {"hold": tight if cam["fw_mode"] == "tight" else _with_sentinels(rng, tight),
                       "not-holding": _rects_that_do_not_hold(rng, F, M, W, H)}
    return cam


def case(seed, calib, n_cams=1, max_masks=256):
    """dict(seed, frames, sizes, inside, layout, cams): frames of float32 [N,4] points and n_cams cameras over them (camera k's case
    covers its first cams[k]["F"] frames)."""
    rng = np.random.default_rng(seed)
    _, T, K0, W0, H0 = S.default_calibration(calib)
    sizes, layout, dense, lead = _frame_sizes(seed, rng)
    inside = [float(rng.choice(INSIDE, p=INSIDE_WEIGHTS)) for _ in sizes]
    if dense is not None:
        inside[dense] = 0.9
    if lead is not None and inside[lead] == 0.0:              # (the one frame no budget drops keeps points inside the image)
        inside[lead] = 0.9
    frames = [np.ascontiguousarray(_frustum_cloud(rng, n, T, np.asarray(K0)[:3, :3], W0, H0, fr), dtype=np.float32).reshape(-1, 4)
              for n, fr in zip(sizes, inside)]
    cams = [_draw_camera(rank(seed) + 7 * k, np.random.default_rng([seed, k + 1]), calib, sizes, max_masks) for k in range(n_cams)]
    return dict(seed=seed, frames=frames, sizes=sizes, inside=inside, layout=layout, cams=cams)


def ladder(calib, image_sizes, seed=77):
    """The deterministic ladder: one batch of LADDER_SIZES points per frame (the last but one takes the second trip of the chunk
    scan), 90 % of them inside the image, 65 masks, box counts cycling through BOX_COUNTS; one camera per (W, H) of image_sizes."""
    rng = np.random.default_rng(seed)
    _, T, K0, W0, H0 = S.default_calibration(calib)
    frames = [np.ascontiguousarray(_frustum_cloud(rng, n, T, np.asarray(K0)[:3, :3], W0, H0, 0.9), dtype=np.float32).reshape(-1, 4)
              for n in LADDER_SIZES]
    cams = []
    for k, size in enumerate(image_sizes):
        crng = np.random.default_rng([seed, k + 1])
        cam = _draw_camera(0, crng, calib, LADDER_SIZES, 256, size=size, M=65)
        assert cam["F"] == len(LADDER_SIZES)
        cam["erode"] = 0                                      # (the masks as drawn: erosion would leave little of the random ones)
        cam["boxes"] = [_draw_boxes(crng, BOX_COUNTS[f % len(BOX_COUNTS)]) for f in range(cam["F"])]
        cams.append(cam)
    return dict(seed=seed, frames=frames, sizes=list(LADDER_SIZES), inside=[0.9] * len(frames), layout="ladder", cams=cams)


def direct_case(M, calib, size=(333, 141), seed=5):
    """The deterministic case of lpf_run_frame_wide's direct form (rectangles, at most 48 masks, a sparse frame): M masks on an
    image whose size is no multiple of 16 and just large enough for the largest frame to count as sparse, shared by frames of 1,
    1023, 1025, 4097 and 20 000 points (90 % inside) and one of 2049 whose first 1024-point chunk lies behind the camera (no valid point: no candidate).  With more than 32 masks the first label
    word's masks are empty -- candidates only in the second word -- and three masks of the last word are empty too, so that the
    word's candidates are no multiple of four.  Rectangles: tight, all "no limit" (on the 20 000-point frame every mask is a candidate
    of every chunk), and not holding."""
    rng = np.random.default_rng([seed, M])
    _, T, K0, W0, H0 = S.default_calibration(calib)
    W, H = size
    sizes = [1, 1023, 1025, 4097, 20000, 2049]
    frames = [np.ascontiguousarray(_frustum_cloud(rng, n, T, np.asarray(K0)[:3, :3], W0, H0, 0.9), dtype=np.float32).reshape(-1, 4) for n in sizes]
    frames[5][:1024, :3] = -np.abs(frames[5][:1024, :3]) - 1.0            # x forward in the velodyne frame: behind the camera
    F = len(sizes)
    one = _draw_masks(rng, 1, M, W, H)[0]
    first = 32 * ((M + 31) // 32 - 1)
    one[:first] = 0
    for i in range(first, M):                                              # every mask of the last word a full, random, rectangle or disk one
        if not one[i].any():
            one[i] = rng.integers(0, 2, size=(H, W), dtype=np.uint8)
    one[first + 1:min(first + 4, M)] = 0                                   # ... but for three (M = 33: the one mask stays)
    member = [one] * F                                                     # (every frame has the same masks)
    tight = np.tile(LpfContext.mask_rects(one)[None], (F, 1, 1))
    cam = dict(T=np.asarray(T, np.float64), K=scaled_K(K0, W0, H0, W, H), W=W, H=H, dmin=0.0, dmax=80.0, M=M, F=F, oriented=True, erode=0,
               kind="u8", binarize="astype", masks=member, member=member, rects=None, rects_mode="none",
               boxes=[_draw_boxes(rng, BOX_COUNTS[f]) for f in range(F)], fw_mode="tight",
               fw_rects={"hold": tight, "no-limit": np.tile(np.array([I32_MIN, I32_MIN, I32_MAX, I32_MAX], np.int32), (F, M, 1)),
                         "not-holding": _rects_that_do_not_hold(rng, F, M, W, H)})
    return dict(seed=seed, frames=frames, sizes=sizes, inside=[0.9] * F, layout="direct", cams=[cam])


# ---- the reference: the C oracle, once per group of 32 masks ------------------------------------------------------------------------
def eroded_member(cam, f, member=None):
    """bool [M,H,W]: frame f's binarised masks after the oracle's erosion"""
    mem = cam["member"][f] if member is None else member
    out = np.zeros(mem.shape, bool)
    for w in range((len(mem) + 31) // 32):
        grp = mem[32 * w:32 * w + 32]
        lab = orc.pack_masks(grp, cam["erode"] if member is None else 0, cam["H"], cam["W"])
        for b in range(len(grp)):
            out[32 * w + b] = (lab >> np.uint32(b)) & np.uint32(1)
    return out


def oracle_result(cam, pts, f, member=None):
    """Frame f's result dict in run_wide's shape (want_float, want_valid_uv) from the oracle, run once per group of 32 masks on the
    binarised masks eroded by the oracle.  member: other binarised masks than the camera's own, not eroded (rectangles that do not
    hold: the masks zeroed outside them)."""
    mem = cam["member"][f] if member is None else member
    erode = cam["erode"] if member is None else 0
    cor = cam["boxes"][f]
    M, N, B = len(mem), len(pts), len(cor)
    LW = (M + 31) // 32
    args = (pts, cam["T"], cam["K"], cam["W"], cam["H"], cam["dmin"], cam["dmax"])
    o = orc.run(*args, corners=cor, oriented=cam["oriented"], want_float=True)
    r = dict(u=o["u"], v=o["v"], depth=o["depth"], uf=o["uf"], vf=o["vf"], valid_idx=o["valid_idx"], n_valid=o["n_valid"],
             label_words=np.zeros((N, LW), np.uint32), inst_lists=[], inst_count=np.zeros(M, np.int64), count_mb=np.zeros((M, B), np.int64),
             best_box=np.full(M, -1, np.int32), best_cnt=np.zeros(M, np.int64))
    for w in range(LW):
        grp = mem[32 * w:32 * w + 32]
        g = orc.run(*args, label_img=orc.pack_masks(grp, erode, cam["H"], cam["W"]), M=len(grp), corners=cor, oriented=cam["oriented"],
                    want_float=False)
        s = slice(32 * w, 32 * w + len(grp))
        r["label_words"][:, w] = g["label_bits"]
        r["inst_lists"] += g["inst_lists"]
        r["inst_count"][s], r["count_mb"][s], r["best_box"][s], r["best_cnt"][s] = g["inst_count"], g["count_mb"], g["best_box"], g["best_cnt"]
    vi = r["valid_idx"]
    r["n_labelled"] = int(r["label_words"].any(axis=1).sum())
    r["label_valid_words"], r["u_valid"], r["v_valid"] = r["label_words"][vi], r["u"][vi], r["v"][vi]
    return r


def common_frames(cs):
    """the frames a multi-camera pass over the case's cameras runs: as many as every camera's masks fit"""
    return min(cam["F"] for cam in cs["cams"])


def reference(cs, k=0):
    """camera k's oracle results of a case, one per frame"""
    cam = cs["cams"][k]
    return [oracle_result(cam, cs["frames"][f], f) for f in range(cam["F"])]


EXACT = ("u", "v", "valid_idx", "label_words", "label_valid_words", "u_valid", "v_valid", "inst_count", "count_mb", "best_box", "best_cnt")
FLOATS = ("depth", "uf", "vf")


def compare(r, ref, what=""):
    """one frame's wide result against oracle_result's, array for array, bit for bit"""
    for k in EXACT:
        assert np.array_equal(r[k], ref[k]), (what, k)
    assert r["n_valid"] == ref["n_valid"] and r["n_labelled"] == ref["n_labelled"], (what, "n_valid, n_labelled")
    assert len(r["inst_lists"]) == len(ref["inst_lists"]), (what, "inst_lists")
    for m, (a, b) in enumerate(zip(r["inst_lists"], ref["inst_lists"])):
        assert np.array_equal(a, b), (what, "inst_lists", m)
    for k in FLOATS:
        assert np.array_equal(r[k], ref[k], equal_nan=True), (what, k)


def check_wide(cam, frames, res, refs, member=None, what="", fresh=True):
    """The checker of the wide fuzz: test_gpu_wide_masks._check (the oracle per group of 32 masks, run afresh) in the camera's depth
    window, then every array against the shared reference ``refs``.  member: as oracle_result's.  fresh=False leaves _check out: for
    a further result of a case whose first result went through it."""
    F = len(refs)
    assert len(res) == F, (what, len(res), F)
    if not fresh:
        pass
    elif member is None:
        _check(cam, res, frames[:F], list(cam["member"]), cam["erode"], cam["boxes"], cam["oriented"], dmin=cam["dmin"], dmax=cam["dmax"])
    else:
        _check(cam, res, frames[:F], list(member), 0, cam["boxes"], cam["oriented"], dmin=cam["dmin"], dmax=cam["dmax"])
    for f in range(F):
        compare(res[f], refs[f], (what, f))


def compare_narrow(r, ref, what=""):
    """one frame of run_cams (run_batch's shape: one label word) against oracle_result's"""
    word = ref["label_words"][:, 0] if ref["label_words"].shape[1] else np.zeros(len(ref["u"]), np.uint32)
    for k in ("u", "v", "valid_idx", "u_valid", "v_valid", "inst_count", "count_mb", "best_box", "best_cnt"):
        assert np.array_equal(r[k], ref[k]), (what, k)
    assert np.array_equal(r["label_bits"], word) and np.array_equal(r["label_valid"], word[ref["valid_idx"]]), (what, "labels")
    assert r["n_valid"] == ref["n_valid"] and r["n_labelled"] == ref["n_labelled"], (what, "n_valid, n_labelled")
    assert len(r["inst_lists"]) == len(ref["inst_lists"]), (what, "inst_lists")
    for m, (a, b) in enumerate(zip(r["inst_lists"], ref["inst_lists"])):
        assert np.array_equal(a, b), (what, "inst_lists", m)
    for k in FLOATS:
        assert np.array_equal(r[k], ref[k], equal_nan=True), (what, k)


def list_needs(refs):
    """entries of every frame's instance lists"""
    return [int(r["inst_count"].sum()) for r in refs]


def tight_inst_cap(refs):
    """an inst_cap below the largest frame's need (None where no frame needs two entries): the frames that need no more fit"""
    needs = list_needs(refs)
    big = max(needs)
    if big < 2:
        return None
    return max(max((n for n in needs if n < big), default=0), big // 2, 1)


def expects_direct(cam, f, n_points, with_rects):
    """lpf_run_frame_wide's routing rule (lpf_api.hip): rectangles, 1..48 masks and a sparse frame take the direct form"""
    return bool(with_rects and 0 < cam["M"] <= 48 and 2 * n_points <= cam["W"] * cam["H"])
