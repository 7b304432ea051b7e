"""Case generator, reference and checker of the seeded differential fuzz of the narrow path (lpf_run_batch, lpf_run_frame, the step
kernel and the mask packs that feed them): tests/test_gpu_fuzz_narrow.py runs the cases on the GPU, tests/test_narrow_fuzz_cases.py
proves on the CPU, from the oracle alone, that the default seeds reach the edges they are meant to reach and that the checker notices
a single wrong entry.  Not a test module.

case(seed, calib) is deterministic from the seed alone.  The values whose presence the CPU test asserts are laid out by the seed's
rank: row seed % 16 of PLAN gives camera size, mask count, mask kind, erosion, mask source, rectangles, box source, output subset,
depth_min and the empty-frame layout (rounds other than the default one, seed // 16 != DEFAULT_SEED_BASE // 16, turn every column of
the row by the round, so other seed bases meet other combinations); the sizes of two frames go by seed % 10; the rest is drawn from
default_rng(seed).

Every camera is the sample camera resampled to another sensor size (wide_fuzz_cases.scaled_K), the clouds come from
test_gpu_fuzz._frustum_cloud at the 1408 x 376 size.  Cases with depth_min != 0 round the depth row of T to multiples of 2^-10: the
generator then places one point per frame whose depth is depth_min EXACTLY, whatever the order of the three products and sums (all
of them are exact in double), inside the image -- a kernel that tests ``>=`` for ``>`` makes it valid.  Under depth_min = -5 a few
points are also placed behind the camera, at depths of -4.9 .. -0.1, inside the image: valid points with a negative depth."""
import os

import numpy as np

import erosion_ref
import wide_fuzz_cases as WG
from lidar_object_detection_amd import synthetic as S
from lidar_object_detection_amd._native import LpfContext
from oracle import cpu_oracle as orc
from oracle import numpy_path as npp
from test_gpu_fuzz import _frustum_cloud
from test_gpu_mask_rects import _outside_zeroed

DEFAULT_CASES = 16                                    # every row of PLAN once
DEFAULT_SEED_BASE = 4000                              # a multiple of 16 and of 10: row k and the frame sizes of seed % 10 belong to seed base + k

CAMERAS = [(1408, 376), (1242, 375), (72, 32), (17, 16), (150, 37), (16, 8), (15, 16), (5, 7)]
DEPTH_MIN = [0.0, 0.5, -5.0]
DEPTH_MAX = WG.DEPTH_MAX
SIZES = [0, 1, 63, 64, 65, 700, 4096, 4097, 9000, 20000]
SIZE_WEIGHTS = np.array([1, 1, 1, 1, 1, 2, 2, 2, 2, 3]) / 16.0
MASK_COUNTS = [0, 1, 3, 8, 9, 16, 17, 32]
KINDS = ["u8", "astype", "v3", "gt0.5"]
ERODE = [0, 1, 2]
ELEMENTS = [3, 5]
SOURCES = ["host", "device", "lent", "lent-unaligned", "label"]
RECTS = ["none", "tight", "sentinel", "not-holding"]
BOX_COUNTS = [0, 1, 7, 33, 64, 65, 130]
BOX_SOURCES = ["velo-host", "velo-device-lent", "cam0", "cam0-visible"]
LAYOUTS = ["drawn", "first", "last", "two", "all", "single"]
# lpf_outputs fields of every output subset (the summary is always asked for; depth, u_f, v_f join on half the seeds)
ALL_FIELDS = ("uv", "label_bits", "valid_idx", "inst_idx", "count_mb", "uv_valid", "label_valid")
OUTPUT_SETS = {"all": ALL_FIELDS,
               "no-uv": tuple(k for k in ALL_FIELDS if k != "uv"),
               "no-label_bits": tuple(k for k in ALL_FIELDS if k != "label_bits"),
               "no-inst_idx": tuple(k for k in ALL_FIELDS if k != "inst_idx"),
               "no-count_mb": tuple(k for k in ALL_FIELDS if k != "count_mb"),
               "valid-only": ("valid_idx", "uv_valid", "label_valid", "inst_idx", "count_mb")}
MASK_BYTES = 70 << 20                                 # uint8 mask bytes of one case: frames are dropped beyond it
FLOAT_ELEMS = WG.FLOAT_ELEMS

# camera, M, kind, erode, element, source, rects, boxes, outputs, depth_min, layout
PLAN = [
    ((1408, 376), 8, "u8", 0, 3, "lent-unaligned", "none", "velo-host", "all", 0.0, "drawn"),          # a size that streams, sent to the tiled pack
    ((1242, 375), 16, "astype", 0, 3, "device", "tight", "cam0-visible", "no-uv", 0.5, "first"),       # odd hw: tiled pack, 2-byte labels
    ((72, 32), 17, "u8", 0, 3, "host", "not-holding", "velo-device-lent", "all", -5.0, "drawn"),       # streaming groups that straddle rows
    ((17, 16), 3, "astype", 0, 3, "lent", "sentinel", "cam0", "no-label_bits", 0.0, "last"),
    ((150, 37), 32, "v3", 1, 5, "host", "not-holding", "velo-host", "no-inst_idx", 0.5, "two"),        # the k x k pack; a hint that must change nothing
    ((16, 8), 1, "u8", 2, 3, "label", "none", "velo-host", "no-count_mb", 0.0, "drawn"),
    ((15, 16), 9, "u8", 0, 3, "device", "not-holding", "cam0-visible", "valid-only", -5.0, "drawn"),   # W < 16: the hint is dropped
    ((5, 7), 17, "u8", 0, 3, "host", "tight", "velo-device-lent", "all", 0.5, "drawn"),                # tiled pack, 4-byte labels
    ((1408, 376), 0, "u8", 1, 3, "lent", "none", "cam0", "all", -5.0, "drawn"),
    ((1242, 375), 1, "u8", 2, 5, "lent-unaligned", "sentinel", "velo-host", "no-uv", 0.0, "all"),
    ((72, 32), 8, "v3", 1, 3, "lent-unaligned", "none", "cam0-visible", "no-label_bits", 0.5, "drawn"),
    ((17, 16), 32, "u8", 0, 3, "label", "none", "velo-device-lent", "no-inst_idx", -5.0, "first"),
    ((150, 37), 9, "u8", 0, 3, "lent-unaligned", "tight", "velo-host", "valid-only", 0.0, "drawn"),
    ((16, 8), 32, "astype", 0, 3, "host", "sentinel", "cam0", "no-count_mb", 0.5, "last"),
    ((15, 16), 16, "gt0.5", 2, 3, "device", "none", "velo-device-lent", "all", -5.0, "two"),
    ((5, 7), 1, "u8", 0, 3, "host", "tight", "cam0-visible", "all", 0.0, "single"),
]
COLUMNS = (CAMERAS, MASK_COUNTS, KINDS, ERODE, ELEMENTS, SOURCES, RECTS, BOX_SOURCES, list(OUTPUT_SETS), DEPTH_MIN, LAYOUTS)


def default_seeds():
    """the seeds of a run without LPF_FUZZ_CASES / LPF_FUZZ_SEED_BASE: the ones the CPU test asserts its conditions over"""
    return [DEFAULT_SEED_BASE + i for i in range(DEFAULT_CASES)]


def seeds():
    """the seeds of this run (LPF_FUZZ_CASES, LPF_FUZZ_SEED_BASE as tests/test_gpu_fuzz.py reads them)"""
    base = int(os.environ.get("LPF_FUZZ_SEED_BASE", str(DEFAULT_SEED_BASE)))
    return [base + i for i in range(int(os.environ.get("LPF_FUZZ_CASES", str(DEFAULT_CASES))))]


def plan(seed):
    """Row seed % 16 of PLAN as a dict; in another round than the default seeds' every column is turned by the round (column j by
    j + 1 places per round), and what the turn makes impossible is settled: a 5 x 5 element needs an image of 16 x 16, a label
    image has no rectangles."""
    row = PLAN[seed % len(PLAN)]
    turn = seed // len(PLAN) - DEFAULT_SEED_BASE // len(PLAN)
    vals = [col[(col.index(v) + turn * (j + 1)) % len(col)] for j, (col, v) in enumerate(zip(COLUMNS, row))]
    p = dict(zip(("size", "M", "kind", "erode", "element", "source", "rects", "boxes", "outs", "dmin", "layout"), vals))
    W, H = p["size"]
    if min(W, H) < 16:
        p["element"] = 3
    if p["source"] == "label" or p["M"] == 0:
        p["rects"] = "none"
    return p


def hint_applies(cs):
    """lpf_set_mask_rects' contract (include/lpf.h): uint8 masks or float masks under "astype", no erosion, an image at least 16
    pixels wide"""
    return cs["rects_mode"] != "none" and cs["kind"] in ("u8", "astype") and cs["erode"] == 0 and cs["W"] >= 16 and cs["M"] > 0


def pack_kind(cs, source=None):
    """Which of pack_masks' three kernels (lpf_api.hip) packs the case's masks, by shape alone: "element" (lpf_pack_erode_k: an
    erosion with another element than 3 x 3), "stream" (lpf_pack16: hw % 16 == 0 and a 16-byte aligned pointer) or "tiled"
    (lpf_pack_erode).  None: nothing is packed (no masks, or a label image is handed over)."""
    source = source or cs["source"]
    if cs["M"] == 0 or source == "label":
        return None
    if cs["erode"] > 0 and cs["element"] != 3:
        return "element"
    return "stream" if (cs["W"] * cs["H"]) % 16 == 0 and source != "lent-unaligned" else "tiled"


def label_bytes(M):
    return 1 if M <= 8 else 2 if M <= 16 else 4


def _frame_sizes(seed, rng, layout):
    """points per frame: F in 1..4 frames of drawn sizes, two of them laid out by seed % 10 -- SIZES[seed % 10] in slot ``lead``
    (frame 0; frame 1 under "first") and SIZES[(seed + 4) % 10] behind it -- where the layout leaves them"""
    F = int(rng.integers(1, 5))
    sizes = [int(rng.choice(SIZES, p=SIZE_WEIGHTS)) for _ in range(4)]
    if layout == "single":
        return [0]
    if layout == "all":
        return [0] * max(F, 2)
    lead = 1 if layout == "first" else 0
    head = lead + 2
    F = min(4, max(F, head + {"drawn": 0, "first": 0, "last": 1, "two": 2}[layout]))
    sizes = [n or 700 for n in sizes[:F]]
    sizes[lead], sizes[lead + 1] = SIZES[seed % len(SIZES)], SIZES[(seed + 4) % len(SIZES)]
    if layout == "first":
        sizes[0] = 0
    elif layout == "last":
        sizes[-1] = 0
    elif layout == "two":
        if F == head + 2:
            sizes[head] = sizes[head + 1] = 0
        else:                                                 # (four frames at the most: the pair takes the second laid-out slot)
            sizes[lead + 1] = sizes[lead + 2] = 0
    return sizes


def _depth_row_rounded(T):
    T = np.array(T, np.float64)
    T[2] = np.round(T[2] * 1024.0) / 1024.0
    return T


def point_at_depth(T, K, W, H, depth):
    """A float32 velodyne point whose depth under T (depth row in multiples of 2^-10) is ``depth`` exactly, close to the ray
    of the image's centre (behind the camera too: u = (fx x + cx z) / |z|): x, y, z are multiples of 2^-10 with 1024 * depth = a X + b Y + c Z + 1024 d solved in integers next to the point of that
    ray at that depth -- every product and sum of the depth is exact in double, in any order and with or without fused
    multiply-adds."""
    a, b, c, d = (int(v) for v in np.round(T[2] * 1024.0))
    cam = np.array([(0.5 * W * abs(depth) - K[0, 2] * depth) / K[0, 0], (0.5 * H * abs(depth) - K[1, 2] * depth) / K[1, 1], depth])
    axis = np.linalg.solve(T[:3, :3], cam - T[:3, 3])
    want = int(round(depth * 1024.0 * 1024.0)) - 1024 * d               # a X + b Y + c Z, X = 1024 x ...
    y0, z0 = int(round(axis[1] * 1024.0)), int(round(axis[2] * 1024.0))
    best = None
    for dy in range(-60, 61):
        for dz in range(-60, 61):
            rest = want - b * (y0 + dy) - c * (z0 + dz)
            if a and rest % a == 0 and (best is None or dy * dy + dz * dz < best[0]):
                best = (dy * dy + dz * dz, rest // a, y0 + dy, z0 + dz)
    assert best is not None, "no lattice point at depth %r" % depth
    p = np.array([best[1] / 1024.0, best[2] / 1024.0, best[3] / 1024.0, 1.0], np.float32)
    assert float(np.dot(T[2, :3], p[:3].astype(np.float64)) + T[2, 3]) == depth
    return p


def _behind(rng, k, T, K, W, H):
    """k float32 points behind the camera (depth -4.9 .. -0.1) that project into the middle of the image"""
    u, v = rng.uniform(0.3 * W, 0.7 * W, k), rng.uniform(0.3 * H, 0.7 * H, k)
    d = -rng.uniform(0.1, 4.9, k)
    cam = np.stack([(u * np.abs(d) - K[0, 2] * d) / K[0, 0], (v * np.abs(d) - K[1, 2] * d) / K[1, 1], d, np.ones(k)])
    out = np.ones((k, 4), np.float32)
    out[:, :3] = np.linalg.solve(T, cam)[:3].T
    return out


def _draw_boxes(rng, B, TrVeloToCam):
    """B cam-0 boxes: wide_fuzz_cases._draw_boxes' velodyne boxes (half of them scaled up, often the last a copy of the first: a
    tie) taken to camera 0"""
    velo = WG._draw_boxes(rng, B)
    homo = np.concatenate([velo.reshape(-1, 3), np.ones((8 * B, 1))], axis=1)
    return np.ascontiguousarray((np.asarray(TrVeloToCam, np.float64) @ homo.T).T[:, :3].reshape(B, 8, 3))


def case(seed, calib, sizes=None, **over):
    """One case as a dict: seed, the plan's values (W, H, M, kind, binarize, erode, element, source, rects_mode, box_source, outs,
    dmin), dmax, T, K, oriented, want_float, tight_cap, sizes, inside, frames (float32 [N,4] each), on_dmin (per frame: index of
    the point at depth == dmin, or -1), masks ([F,M,H,W] uint8 or float32), member ([F,M,H,W] uint8 0/1, the masks binarised),
    rects ([F,M,4] int32 or None), cam0 (per frame [B,8,3] cam-0 corners), Tcv, TrVeloToCam.  ``over`` replaces values of the
    seed's plan (its keys), ``sizes`` the points per frame: for callers that lay out their own cases (tests/sequence_fuzz_cases.py);
    without them the case is the seed's own."""
    rng = np.random.default_rng(seed)
    p = plan(seed)
    if over:
        p.update(over)
        if p["source"] == "label" or p["M"] == 0:
            p["rects"] = "none"
    TrVeloToCam, T, K0, W0, H0 = S.default_calibration(calib)
    K0 = np.asarray(K0, np.float64)[:3, :3]
    T = np.asarray(T, np.float64)
    W, H = p["size"]
    M, dmin = p["M"], p["dmin"]
    if dmin != 0.0:
        T = _depth_row_rounded(T)
    drawn = _frame_sizes(seed, rng, p["layout"])
    sizes = drawn if sizes is None else list(sizes)
    while len(sizes) > 1 and len(sizes) * M * H * W > MASK_BYTES:
        sizes.pop()
    F = len(sizes)
    inside = [float(rng.choice(WG.INSIDE, p=WG.INSIDE_WEIGHTS)) for _ in sizes]
    lead = 1 if p["layout"] == "first" else 0
    for f in (lead, lead + 1):                                # the laid-out frames keep points inside the image
        if f < F and inside[f] == 0.0:
            inside[f] = 0.9
    frames, on_dmin = [], []
    for n, fr in zip(sizes, inside):
        pts = np.ascontiguousarray(_frustum_cloud(rng, n, T, K0, W0, H0, fr), dtype=np.float32).reshape(-1, 4)
        at = -1
        if dmin != 0.0 and n >= 63:
            at = n // 2
            pts[at] = point_at_depth(T, K0, W0, H0, dmin)
            if dmin < 0.0:
                pts[n // 3:n // 3 + 4] = _behind(rng, 4, T, K0, W0, H0)
        frames.append(pts)
        on_dmin.append(at)
    u8 = WG._draw_masks(rng, F, M, W, H)
    kind = p["kind"] if F * M * H * W <= FLOAT_ELEMS else "u8"
    if kind == "u8":
        masks, member, binarize = u8 * np.uint8(rng.choice([1, 200, 255])), u8, "astype"
    else:
        masks = u8.astype(np.float32)
        for f in range(F):
            if M:
                masks[f, int(rng.integers(0, M))] *= rng.choice(WG.ODD, size=(H, W))
        member, binarize = orc.binarize_f32(masks, WG.RULES.index(kind)), kind
    member = (member != 0).astype(np.uint8)
    mode = p["rects"]
    tight = LpfContext.mask_rects(member) if M else np.zeros((F, 0, 4), np.int32)
    rects = {"none": lambda: None, "tight": lambda: tight, "sentinel": lambda: WG._with_sentinels(rng, tight),
             "not-holding": lambda: WG._rects_that_do_not_hold(rng, F, M, W, H)}[mode]()
    B0 = BOX_COUNTS[seed % len(BOX_COUNTS)]
    cam0 = [_draw_boxes(rng, B0 if f == 0 else int(rng.choice(BOX_COUNTS)), TrVeloToCam) for f in range(F)]
    if p["boxes"] == "cam0-visible":
        for c in cam0:
            c[1::5, :, 2] *= -1.0                             # every fifth box behind the camera: filter_visible has boxes to drop
    return dict(seed=seed, W=W, H=H, M=M, F=F, kind=kind, binarize=binarize, erode=p["erode"], element=p["element"], source=p["source"],
                rects_mode=mode, box_source=p["boxes"], outs=p["outs"], layout=p["layout"], dmin=dmin, dmax=float(rng.choice(DEPTH_MAX)),
                T=T, K=WG.scaled_K(K0, W0, H0, W, H), oriented=bool(rng.integers(0, 2)), want_float=bool((seed // 2) % 2),
                tight_cap=bool(seed % 2), sizes=sizes, inside=inside, frames=frames, on_dmin=on_dmin, masks=masks, member=member,
                rects=rects, cam0=cam0, TrVeloToCam=np.asarray(TrVeloToCam, np.float64), Tcv=np.linalg.inv(np.asarray(TrVeloToCam, np.float64)))


def fields(cs):
    """the lpf_outputs fields the case asks for"""
    return OUTPUT_SETS[cs["outs"]] + (("depth", "u_f", "v_f") if cs["want_float"] else ())


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def reference_members(cs, hint=True):
    """uint8 0/1 [F,M,H,W]: the masks as the library has to read them -- binarised; zeroed outside rectangles that do not hold where
    the hint applies (everywhere else the hint changes nothing)"""
    member = cs["member"]
    if hint and cs["rects_mode"] == "not-holding" and hint_applies(cs):
        member = _outside_zeroed(member, WG.clipped(cs["rects"], cs["W"], cs["H"]))
    return member


def label_images(cs, hint=True):
    """uint32 [F,H,W]: the reference label images -- reference_members eroded (the 3 x 3 cross by the oracle, another element by
    tests/erosion_ref.py) and packed by the oracle"""
    member = reference_members(cs, hint)
    H, W = cs["H"], cs["W"]
    out = np.zeros((cs["F"], H, W), np.uint32)
    for f in range(cs["F"]):
        if cs["M"] == 0:
            continue
        if cs["erode"] and cs["element"] != 3:
            out[f] = orc.pack_masks(erosion_ref.erode(member[f], cs["element"], cs["erode"]), 0, H, W)
        else:
            out[f] = orc.pack_masks(member[f], cs["erode"], H, W)
    return out


def reference(cs, hint=True):
    """One dict per frame from the C oracle (orc.run on the reference label image): orc.run's keys, u_valid, v_valid, label_valid,
    n_labelled, need (entries of all instance lists), label_img (the frame's reference label image) and ``visible`` (bool [B_f]: the
    boxes kept).  The boxes are npp.prepare_boxes'
    velodyne corners of the cam-0 corners; under "cam0-visible" the oracle sees the kept boxes only and count_mb / best_box are
    mapped back to the given list, as tests/test_gpu_perrun.py does: dropped boxes count zero."""
    labels = label_images(cs, hint)
    refs = []
    for f in range(cs["F"]):
        cam0 = cs["cam0"][f]
        B = len(cam0)
        keep, velo = npp.prepare_boxes(cam0, cs["K"], cs["W"], cs["H"], cs["TrVeloToCam"])
        if cs["box_source"] != "cam0-visible":
            keep = np.ones(B, bool)
        o = orc.run(cs["frames"][f], cs["T"], cs["K"], cs["W"], cs["H"], cs["dmin"], cs["dmax"], label_img=labels[f] if cs["M"] else None,
                    M=cs["M"], corners=velo[keep], oriented=cs["oriented"], want_float=True)
        del o["inst_idx"]
        pos = np.flatnonzero(keep)
        full = np.zeros((cs["M"], B), np.int64)
        full[:, keep] = o["count_mb"]
        o["count_mb"] = full
        o["best_box"] = np.where(o["best_box"] >= 0, pos[np.maximum(o["best_box"], 0)] if len(pos) else -1, -1).astype(np.int32)
        vi = o["valid_idx"]
        o.update(u_valid=o["u"][vi], v_valid=o["v"][vi], label_valid=o["label_bits"][vi], n_labelled=int(np.count_nonzero(o["label_bits"])),
                 need=int(o["inst_count"].sum()), visible=keep, corners_velo=velo, inst_overflow=0, label_img=labels[f])
        refs.append(o)
    return refs


def tight_inst_cap(refs):
    """wide_fuzz_cases.tight_inst_cap over the narrow reference: below the largest frame's need, the others fit"""
    return WG.tight_inst_cap(refs)


EXACT = ("u", "v", "label_bits", "valid_idx", "u_valid", "v_valid", "label_valid", "inst_count", "count_mb", "best_box", "best_cnt")
SCALARS = ("n_valid", "n_labelled", "inst_overflow")
FLOATS = ("depth", "uf", "vf")
KEYS = EXACT + SCALARS + FLOATS + ("inst_lists", "visible")


def check(cs, got, refs, route="", inst_cap=None):
    """Every output that ``got`` (one dict per frame, keys as LpfContext.run_batch names them; optional: inst_overflow, visible) holds
    against the reference, bit for bit; the failing assertion names the seed, route, frame and key.  inst_cap: the capacity the run
    had where it does not run again on overflow -- a frame that needs more has inst_overflow = 1 and its lists are not compared
    (include/lpf.h says "lists truncated", not what a truncated list holds); everything else of the frame is."""
    seed = cs["seed"]
    assert len(got) == len(refs), (seed, route, "frames", len(got), len(refs))
    for f, (r, ref) in enumerate(zip(got, refs)):
        unknown = set(r) - set(KEYS)
        assert not unknown, (seed, route, f, sorted(unknown))
        over = inst_cap is not None and ref["need"] > inst_cap
        for k in EXACT:
            if k in r:
                assert np.array_equal(r[k], ref[k]), (seed, route, f, k)
        for k in SCALARS:
            if k in r:
                assert int(r[k]) == (int(over) if k == "inst_overflow" else ref[k]), (seed, route, f, k)
        for k in FLOATS:
            if k in r:
                assert np.array_equal(r[k], ref[k], equal_nan=True), (seed, route, f, k)
        if "visible" in r:
            assert np.array_equal(np.asarray(r["visible"], bool), ref["visible"]), (seed, route, f, "visible")
        if "inst_lists" in r and not over:
            assert len(r["inst_lists"]) == len(ref["inst_lists"]), (seed, route, f, "inst_lists")
            for m, (a, b) in enumerate(zip(r["inst_lists"], ref["inst_lists"])):
                assert np.array_equal(a, b), (seed, route, f, "inst_lists", m)
