"""Case generator of the seeded differential fuzz over the COMPACT mask forms -- run-length masks (rle.RleMasks) and instance-ID maps
(idmap.IdMasks, uint16 and int32) -- alone and in sequences of calls on one context: tests/test_gpu_fuzz_forms.py runs the cases on
the GPU, tests/test_form_fuzz_cases.py proves on the CPU, from the oracle and this module alone, that the default seeds reach the
edges they are meant to reach and that the checkers notice a single wrong entry.  Not a test module.

case(seed, calib) is deterministic from the seed.  Row seed % 16 of PLAN lays out what the CPU test counts (form, camera, mask count,
erosion, element, where an ID map lives and how many elements past its allocation it starts, the pending hint, the fewest frames --
once for the narrow route and once for the wide routes); the rest is drawn from default_rng(seed).  Other rounds than the default
seeds' (seed // 16) turn the form, the offset k and the erosion by the round.

The yardstick is the existing one, unchanged: a case is narrow_fuzz_cases.case (cameras, clouds, boxes, depth window, empty-frame
layout, output subset) resp. wide_fuzz_cases' frames and _draw_camera, with ``member`` REPLACED by the membership the compact form
encodes, so narrow_fuzz_cases.reference / check / label_images and wide_fuzz_cases.oracle_result / check_wide run on the equivalent
dense masks (the C oracle).  The encoders under test are not their own yardstick: runs come from tests/rle_ref.py's canonical runs of
the member masks (never RleMasks.from_dense) and are then perturbed without changing membership -- the module asserts
rle_ref.masks_to_dense(perturbed) == member for every frame it emits; an ID map's membership is restated here as
``(ids.astype(int64) == sel[m]) & (sel[m] != LPF_ID_NONE)`` (for a uint16 map: and 0 <= sel[m] <= 65535) and asserted equal to
IdMasks.to_dense().

Cameras: narrow_fuzz_cases.CAMERAS, 37 x 23 (851 pixels: odd, at least 16 wide) and 3 x 2 -- the only size at which a frame of an ID
map has NO whole 16-byte group (lpf_ids.hip.h: nvec == 0; 5 x 7 always has three or more)."""
import os

import numpy as np

import narrow_fuzz_cases as NG
import rle_ref as R
import wide_fuzz_cases as WG
from lidar_object_detection_amd import synthetic as S
from lidar_object_detection_amd.idmap import LPF_ID_NONE, IdMasks
from lidar_object_detection_amd.rle import RleMasks
from test_gpu_fuzz import _frustum_cloud

DEFAULT_CASES = 16                                    # every row of PLAN once
DEFAULT_SEED_BASE = 9600                              # a multiple of 16
FORMS = ("rle", "ids-uint16", "ids-int32")
ODD, TINY = (37, 23), (3, 2)
CAMERAS = NG.CAMERAS + [ODD, TINY]
BIG = [(1408, 376), (1242, 375)]
NARROW_COUNTS = [0, 1, 8, 9, 16, 17, 31, 32]
WIDE_COUNTS = [1, 32, 33, 64, 65, 255, 256]
ID_SOURCES = ("host", "device", "device-offset")
ID_DTYPES = {"ids-uint16": np.uint16, "ids-int32": np.int32}
POOLS = {"ids-uint16": [0, 1, 65535], "ids-int32": [LPF_ID_NONE, -1, 0, 65536, 65541, 2 ** 31 - 1]}
MID_RANGE = {"ids-uint16": (2, 65535), "ids-int32": (-(1 << 30), 1 << 30)}
SPLITS = (1023, 1024, 1025, 2049)                     # a run longer than this is cut at start + this: lpf_rle.hip.h cuts units at 1024 pixels
CHUNK = 1024                                          # LPF_RLE_CHUNK
PERTURBATIONS = ("none", "split", "split-long", "zero-length", "repeat", "overlap", "shuffle", "all")
MAX_RUNS = 20000                                      # runs per mask: a mask with more keeps a band of six rows (the full-size cameras' random masks)
MAX_POINTS = 9000                                     # points per frame of the wide routes

# narrow: form, camera, M, erode, element, ID source, k, hint, fewest frames | wide: form, camera, M, ID source, k
PLAN = [
    ("rle", (1408, 376), 8, 0, 3, None, 0, True, 2, "ids-uint16", (150, 37), 33, "device-offset", 3),
    ("ids-uint16", ODD, 9, 0, 3, "device-offset", 1, True, 4, "rle", ODD, 64, None, 0),
    ("ids-int32", (5, 7), 17, 0, 3, "device-offset", 1, False, 4, "ids-int32", (17, 16), 256, "host", 0),
    ("rle", ODD, 8, 1, 3, None, 0, False, 3, "ids-uint16", ODD, 255, "device-offset", 3),
    ("ids-uint16", (150, 37), 32, 1, 5, "host", 0, False, 2, "rle", (1242, 375), 33, None, 0),
    ("ids-int32", (16, 8), 1, 2, 3, "device", 0, False, 2, "rle", (150, 37), 256, None, 0),
    ("rle", (5, 7), 16, 0, 3, None, 0, False, 3, "ids-int32", ODD, 65, "device-offset", 1),
    ("ids-uint16", TINY, 8, 0, 3, "device-offset", 5, False, 2, "ids-int32", TINY, 32, "device-offset", 1),
    ("rle", (72, 32), 31, 2, 5, None, 0, False, 3, "ids-uint16", (1408, 376), 32, "device", 0),
    ("ids-int32", (1242, 375), 8, 0, 3, "host", 0, True, 2, "rle", (72, 32), 65, None, 0),
    ("ids-uint16", (17, 16), 0, 0, 3, "host", 0, False, 2, "ids-int32", (150, 37), 64, "device-offset", 2),
    ("rle", ODD, 9, 0, 3, None, 0, False, 3, "ids-uint16", (5, 7), 1, "host", 0),
    ("ids-int32", ODD, 16, 1, 3, "device-offset", 3, False, 4, "rle", (17, 16), 255, None, 0),
    ("rle", (150, 37), 32, 0, 3, None, 0, True, 3, "ids-int32", (72, 32), 33, "device", 0),
    ("ids-uint16", (72, 32), 17, 2, 3, "device", 0, False, 3, "ids-uint16", ODD, 256, "device-offset", 6),
    ("ids-int32", (15, 16), 31, 0, 3, "host", 0, False, 3, "rle", (5, 7), 32, None, 0),
]
KEYS = ("form", "size", "M", "erode", "element", "source", "k", "hint", "frames", "wform", "wsize", "wM", "wsource", "wk")


def default_seeds():
    """the seeds of a run without LPF_FUZZ_CASES / LPF_FUZZ_SEED_BASE: the ones the CPU test asserts its conditions over"""
    return [DEFAULT_SEED_BASE + i for i in range(DEFAULT_CASES)]


def seeds():
    """the seeds of this run (LPF_FUZZ_CASES, LPF_FUZZ_SEED_BASE as tests/test_gpu_fuzz.py reads them)"""
    base = int(os.environ.get("LPF_FUZZ_SEED_BASE", str(DEFAULT_SEED_BASE)))
    return [base + i for i in range(int(os.environ.get("LPF_FUZZ_CASES", str(DEFAULT_CASES))))]


def per(form):
    """elements of an ID map per 16-byte group (lpf_ids.hip.h: PER)"""
    return 16 // np.dtype(ID_DTYPES[form]).itemsize


def plan(seed):
    """Row seed % 16 of PLAN as a dict.  In another round than the default seeds' the forms turn by the round (a form's ID source
    goes with it: an ID form that takes over a run-length slot reads a device map), the offsets k by the round modulo PER, and the
    erosion of the rows without a hint by the round modulo 3; the cameras and mask counts stay (the full-size cameras keep their few
    masks)."""
    p = dict(zip(KEYS, PLAN[seed % len(PLAN)]))
    turn = seed // len(PLAN) - DEFAULT_SEED_BASE // len(PLAN)
    if turn:
        for fk, sk, kk in (("form", "source", "k"), ("wform", "wsource", "wk")):
            p[fk] = FORMS[(FORMS.index(p[fk]) + turn) % 3]
            if p[fk] == "rle":
                p[sk], p[kk] = None, 0
            else:
                p[sk] = p[sk] or "device-offset"
                p[kk] = (p[kk] + turn) % per(p[fk]) if p[sk] == "device-offset" else 0
        if not p["hint"]:
            p["erode"] = (p["erode"] + turn) % 3
    if min(p["size"]) < 16:
        p["element"] = 3
    return p


def label_bytes(M):
    return NG.label_bytes(M)


def splits(hw, F, k, itemsize):
    """[(head, nvec, tail)] per frame of an ID map of F frames of hw elements that starts k elements behind a 16-byte boundary
    (lpf_ids.hip.h, lpf_ids_split, restated): the elements before the first boundary, the whole groups, the rest"""
    PER = 16 // itemsize
    out = []
    for f in range(F):
        addr = (k + f * hw) * itemsize
        head = min(((16 - addr % 16) % 16) // itemsize, hw)
        nvec = (hw - head) // PER
        out.append((head, nvec, hw - head - nvec * PER))
    return out


# ---- membership: what both forms encode -----------------------------------------------------------------------------------------------
def _tame(member, size):
    """The drawn member masks made affordable: a mask of more than MAX_RUNS runs keeps a band of six rows, and at a full-size camera
    only the first full mask of the case stays full (one run of H * W pixels is 517 work units there): the others keep their middle."""
    F, M, H, W = member.shape
    full_seen = False
    for f in range(F):
        for m in range(M):
            pl = member[f, m]
            if size in BIG and pl.all():
                if full_seen:
                    pl[:] = 0
                    pl[H // 4:H // 2, W // 4:W // 2] = 1
                full_seen = True
            elif int(np.count_nonzero(np.diff(pl.reshape(-1).astype(np.int8)) == 1)) > MAX_RUNS:
                y0 = (7 * m + 3 * f) % max(H - 6, 1)
                keep = pl[y0:y0 + 6].copy()
                pl[:] = 0
                pl[y0:y0 + 6] = keep
    return member


def mask_counts(rng, seed, F, M):
    """masks per frame: M, but for one frame with fewer (drawn) on half the seeds, and one frame with NONE where seed % 4 says so --
    1: the first, 2: the last, 3: a middle one (the first where there are fewer than three frames)"""
    counts = [M] * F
    if M and rng.random() < 0.5:
        counts[int(rng.integers(0, F))] = int(rng.integers(0, M))
    where = seed % 4
    if M and F >= 2 and where:
        counts[{1: 0, 2: F - 1, 3: F // 2 if F >= 3 else 0}[where]] = 0
    if M and max(counts) < M:                                 # (some frame keeps all M: the batch's mask count is the plan's)
        counts[1 if counts[0] == 0 else 0] = M
    return counts


def _runless(seed, f, n):
    """the masks of a frame of n >= 4 masks that get NO run: the first (f % 3 == 0), the last two (1) or the second and third (2) --
    the equal offsets of the decode's owner search at position 0, at M - 1 and in consecutive positions"""
    if n < 4:
        return []
    return [[0], [n - 2, n - 1], [1, 2]][(f + seed) % 3]


def rle_members(rng, seed, member, counts):
    """The member masks a run-length case encodes: the drawn ones, a frame's masks beyond its count empty (padding), the run-less masks
    of _runless empty, one mask of a case with 2304 pixels or more full, and the LAST pixel of every frame that has runs a member of the
    frame's first mask with runs (a run that ends on the last pixel: the word shared with the next frame where H * W is no multiple of
    the elements per word)."""
    F, M, H, W = member.shape
    out = member.copy()
    for f in range(F):
        n = counts[f]
        out[f, n:] = 0
        skip = _runless(seed, f, n)
        out[f, skip] = 0
        first = next((m for m in range(n) if m not in skip), None)
        if first is not None:
            out[f, first, H - 1, W - 1] = 1
            if f == 0 and H * W >= 2304 and n >= 2:
                out[f, n - 1 if n - 1 not in skip else first] = 1      # one run of H * W pixels
    return out


def _perturb(rng, runs, kind, hw, cut):
    """one mask's canonical runs [(start, length)] perturbed without changing membership"""
    runs = list(runs)
    if kind in ("split", "all"):
        out = []
        for s, n in runs:
            if n >= 2 and rng.random() < 0.5:
                a = int(rng.integers(1, n))
                out += [(s, a), (s + a, n - a)]
            else:
                out.append((s, n))
        runs = out
    if kind in ("split-long", "all"):
        out = []
        for s, n in runs:
            if n > cut:
                out += [(s, cut), (s + cut, n - cut)]
            else:
                out.append((s, n))
        runs = out
    if kind in ("repeat", "all") and runs:
        for i in rng.integers(0, len(runs), size=min(3, len(runs))):
            runs.insert(int(rng.integers(0, len(runs) + 1)), runs[int(i)])
    if kind in ("overlap", "all"):
        out = []
        for s, n in runs:
            if n >= 3 and rng.random() < 0.5:
                b = int(rng.integers(1, n - 1))
                a = int(rng.integers(b + 1, n + 1))
                out += [(s, a), (s + b, n - b)]                       # [s, s + a) and [s + b, s + n) share [s + b, s + a)
            else:
                out.append((s, n))
        runs = out
    if kind in ("shuffle", "all") and len(runs) > 1:
        runs = [runs[int(i)] for i in rng.permutation(len(runs))]
    if kind in ("zero-length", "all"):
        runs.insert(0, (0, 0))
        runs.insert(len(runs) // 2 + 1 if len(runs) > 1 else 1, (hw // 2, 0))
        runs.append((hw, 0))
    return runs


def encode_rle(rng, seed, member, counts, runless=True):
    """([RleMasks per frame], [per frame: per mask its perturbation]) of uint8 [F,M,H,W] member masks: frame f has counts[f] masks,
    each tests/rle_ref.py's canonical runs under perturbation (f * M + m + seed) % 8 of PERTURBATIONS, "split-long" at
    start + SPLITS[(f + m) % 4].  A mask without members gets no run, unless its perturbation is "zero-length" or "all" and it is not
    one of _runless' masks (runless=False: members that were not laid out by rle_members, no such masks).  Asserts that the runs decode to the member masks (rle_ref.masks_to_dense)."""
    F, M, H, W = member.shape
    hw = H * W
    frames, kinds = [], []
    for f in range(F):
        n = counts[f]
        skip = _runless(seed, f, n) if runless else []
        per_mask, kk = [], []
        for m in range(n):
            kind = PERTURBATIONS[(f * M + m + seed) % len(PERTURBATIONS)]
            canon = R.dense_to_runs_fast(member[f, m])
            if m in skip:
                assert not canon
                kind = "none"
            per_mask.append(_perturb(rng, canon, kind, hw, SPLITS[(f + m) % len(SPLITS)]))
            kk.append(kind)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum([len(r) for r in per_mask])
        flat = np.array([r for rs in per_mask for r in rs], np.int32).reshape(-1, 2)
        assert np.array_equal(R.masks_to_dense(flat, off, n, H, W), member[f, :n]) and not member[f, n:].any(), (seed, f, "runs")
        frames.append(RleMasks(flat, off, (n, H, W)))
        kinds.append(kk)
    return frames, kinds


def _instance_ids(rng, form, n):
    """n + 1 distinct IDs of the form's type, the LAST ones from the form's pool (both ends of the type: the masks painted last are
    the ones least hidden), the others mid-range; the last of all is the background's"""
    pool = list(POOLS[form])
    lo, hi = MID_RANGE[form]
    mid = []
    while len(mid) < max(n + 1 - len(pool), 0):
        v = int(rng.integers(lo, hi))
        if v not in pool and v not in mid:
            mid.append(v)
    ids = mid + [pool[int(i)] for i in rng.permutation(len(pool))]
    return np.array(ids[len(ids) - (n + 1):], np.int64)


def _absent(rng, form, present):
    lo, hi = MID_RANGE[form]
    while True:
        v = int(rng.integers(lo, hi))
        if v not in present:
            return v


def encode_ids(rng, seed, form, member, counts):
    """(ids [F,H,W] of the form's type, [sel int64 per frame], [per frame: what its table holds]) of uint8 [F,M,H,W] drawn masks: the
    map is painted mask by mask, the later mask winning, over a background ID.  Frame f's table has counts[f] entries: a shuffled
    subset of the painted IDs, then -- where the table is long enough -- a duplicate (entry 1 = entry 0), an ID the map does not hold
    (entry 2), for a uint16 map -1, 65536 or 65536 + a present ID (entry 3, and another of the three as entry 5), LPF_ID_NONE (entry 4); the background's ID as the last
    entry of frame 0 where seed % 4 == 2; and on odd seeds the last frame's entries all replaced by IDs that select nothing."""
    F, M, H, W = member.shape
    dt = ID_DTYPES[form]
    ids = np.zeros((F, H, W), np.int64)
    sels, holds = [], []
    for f in range(F):
        pid = _instance_ids(rng, form, M)
        bg = int(pid[M])
        img = np.full((H, W), bg, np.int64)
        for m in range(M):
            img[member[f, m] != 0] = pid[m]
        ids[f] = img
        present = set(int(v) for v in np.unique(img))
        n = counts[f]
        sel = pid[rng.permutation(M)[:n]].astype(np.int64)
        has = set()
        if n >= 2:
            sel[1] = sel[0]
            has.add("duplicate")
        if n >= 3:
            sel[2] = _absent(rng, form, present | set(int(v) for v in pid))
            has.add("absent")
        if n >= 4 and form == "ids-uint16":
            some = sorted(present)[int(rng.integers(0, len(present)))]
            sel[3] = (-1, 65536, 65536 + some)[(f + seed) % 3]
            has.add("out-of-range")
            if n >= 6:
                sel[5] = (-1, 65536, 65536 + some)[(f + seed + 1) % 3]
        if n >= 5:
            sel[4] = LPF_ID_NONE
            has.add("none-entry")
        if n and f == 0 and seed % 4 == 2:
            sel[n - 1] = bg
            has.add("background")
        if n and F >= 2 and f == F - 1 and seed % 2 == 1:
            for j in range(n):
                sel[j] = (LPF_ID_NONE, _absent(rng, form, present), -1 if form == "ids-uint16" else _absent(rng, form, present))[j % 3]
            has = {"nothing-selected"}
        sels.append(sel)
        holds.append(has)
    assert ids.min() >= np.iinfo(dt).min and ids.max() <= np.iinfo(dt).max
    return ids.astype(dt), sels, holds


def ids_members(ids, sels, M):
    """uint8 [F,M,H,W]: the membership an ID map and its tables encode, restated -- mask m = the pixels whose ID, as an integer,
    equals sel[m]; LPF_ID_NONE selects nothing, and neither does an entry outside 0 .. 65535 in a uint16 map; a frame's entries beyond
    its table are LPF_ID_NONE (padding).  Asserted equal to IdMasks.to_dense()."""
    F, H, W = ids.shape
    out = np.zeros((F, M, H, W), np.uint8)
    wide = ids.astype(np.int64)
    for f, sel in enumerate(sels):
        for m, v in enumerate(sel):
            v = int(v)
            in_range = ids.dtype != np.uint16 or 0 <= v <= 65535
            out[f, m] = (wide[f] == v) & (v != LPF_ID_NONE) & in_range
        assert np.array_equal(IdMasks(ids[f], sel).to_dense(), out[f, :len(sel)]), (f, "IdMasks.to_dense")
    return out


def encode(rng, seed, form, drawn, counts, size):
    """the compact form of a case's drawn masks: dict(form, member [F,M,H,W] uint8 -- what the form encodes --, counts, and rle
    (frames of RleMasks), kinds -- or ids, sel, holds)"""
    drawn = _tame((np.asarray(drawn) != 0).astype(np.uint8), size)
    M = drawn.shape[1]
    if form == "rle":
        member = rle_members(rng, seed, drawn, counts)
        rle, kinds = encode_rle(rng, seed, member, counts)
        return dict(form=form, member=member, counts=counts, rle=rle, kinds=kinds)
    ids, sels, holds = encode_ids(rng, seed, form, drawn, counts)
    return dict(form=form, member=ids_members(ids, sels, M), counts=counts, ids=ids, sel=sels, holds=holds)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------
def _narrow_sizes(seed, rng, layout, size, fewest):
    sizes = NG._frame_sizes(seed, np.random.default_rng(seed), layout)
    while len(sizes) < fewest:
        sizes.append(int(rng.choice(NG.SIZES[1:], p=NG.SIZE_WEIGHTS[1:] / NG.SIZE_WEIGHTS[1:].sum())))
    return sizes[:2] if size in BIG else sizes[:4]


def narrow_case(seed, calib, **over):
    """The narrow case of a seed: narrow_fuzz_cases.case at the plan's camera, mask count, erosion and element with uint8 host masks,
    ``member`` / ``masks`` replaced by the compact form's membership (the dense twin), plus ``compact`` (encode's dict), ``source`` and
    ``k`` of an ID map, and ``hint``: a pending lpf_set_mask_rects hint of rectangles that do NOT hold goes in front of the compact
    setter, which consumes and ignores it (include/lpf.h) -- cs["rects"] holds them, the reference is hint=False."""
    p = dict(plan(seed), **over)
    rng = np.random.default_rng([seed, 101])
    layout = NG.plan(seed)["layout"]
    if layout in ("all", "single"):
        layout = "drawn"
    sizes = _narrow_sizes(seed, rng, layout, p["size"], p["frames"])
    cs = NG.case(seed, calib, sizes=sizes, size=p["size"], M=p["M"], kind="u8", erode=p["erode"], element=p["element"], source="host",
                 rects="not-holding" if p["hint"] else "none", layout=layout)
    counts = mask_counts(rng, seed, cs["F"], cs["M"])
    comp = encode(rng, seed, p["form"], cs["member"], counts, p["size"])
    cs.update(member=comp["member"], masks=comp["member"], compact=comp, form=p["form"], ids_source=p["source"], k=p["k"], hint=bool(p["hint"]))
    assert not cs["hint"] or (cs["rects"] is not None and cs["rects_mode"] == "not-holding")
    return cs


def narrow_reference(cs):
    """narrow_fuzz_cases.reference with the hint ignored: a compact setter consumes a pending hint and ignores it"""
    return NG.reference(cs, hint=False)


def _wide_frames(seed, calib, F):
    """F frames of points as wide_fuzz_cases.case draws them (its _frame_sizes, layout and clouds), at most MAX_POINTS each"""
    rng = np.random.default_rng(seed)
    _, T, K0, W0, H0 = S.default_calibration(calib)
    sizes, layout, _, _ = WG._frame_sizes(seed, rng)
    sizes = [min(n, MAX_POINTS) for n in sizes]
    while len(sizes) < F:
        sizes.append(int(rng.choice(WG.SIZES[1:12])))
    sizes = sizes[:F]
    if not any(sizes):
        sizes[0] = 1025
    inside = [float(rng.choice(WG.INSIDE, p=WG.INSIDE_WEIGHTS)) for _ in sizes]
    inside[int(np.argmax(sizes))] = 0.9
    frames = [np.ascontiguousarray(_frustum_cloud(rng, n, T, np.asarray(K0)[:3, :3], W0, H0, fr), dtype=np.float32).reshape(-1, 4)
              for n, fr in zip(sizes, inside)]
    return frames, sizes, inside, layout


def _compact_camera(seed, k, rng, calib, sizes, size, M, form, element3=True):
    cam = WG._draw_camera(WG.rank(seed) + 7 * k, rng, calib, sizes, 256, size=size, M=M)
    assert cam["F"] == len(sizes)
    counts = mask_counts(rng, seed + k, cam["F"], M)
    comp = encode(rng, seed + k, form, cam["member"], counts, size)
    cam.update(kind="u8", binarize="astype", masks=comp["member"], member=comp["member"], rects=None, rects_mode="none", compact=comp, form=form)
    return cam


def wide_case(seed, calib):
    """The wide case of a seed, in wide_fuzz_cases.case's shape: frames, and cams = [the plan's camera in its compact form, a DENSE
    camera of another size beside it (run_cams_wide; its first 32 masks: run_cams)].  The compact camera also carries ``rle_all``, the
    run-length form of its membership whatever its own form is (run_cams, run_cams_wide, depth_maps take run-length masks; run_cams its
    first 32: ``rle[:32]``), ``ids_source`` and ``k``.  Plus
    the two analysis calls' inputs: ``depth`` (cap: below the largest frame's need on odd seeds) and ``first`` (run-length masks of
    their OWN size, smaller than the camera in one axis and larger in the other, and colours)."""
    p = plan(seed)
    size, M, form = p["wsize"], p["wM"], p["wform"]
    F = 2 if size in BIG else 4 if M <= 65 else 3
    frames, sizes, inside, layout = _wide_frames(seed, calib, F)
    rng = np.random.default_rng([seed, 202])
    cam = _compact_camera(seed, 0, rng, calib, sizes, size, M, form)
    cam.update(ids_source=p["wsource"], k=p["wk"])
    cam["rle_all"] = cam["compact"]["rle"] if form == "rle" else encode_rle(rng, seed + 5, cam["member"], cam["compact"]["counts"], runless=False)[0]
    other = next(s for s in [(70, 33), (17, 16), (150, 37)] if s != size)
    dense = WG._draw_camera(WG.rank(seed) + 7, np.random.default_rng([seed, 203]), calib, sizes, 256, size=other, M=(40, 33, 8)[seed % 3])
    # first_match: masks at their own size
    W, H = size
    mw, mh = (max(W - 5, 1), H + 3) if seed % 2 else (W + 4, max(H - 1, 1))
    fm_M = (1, 33, 9, 40)[seed % 4]
    fm_drawn = WG._draw_masks(rng, F, fm_M, mw, mh)
    fm_counts = mask_counts(rng, seed + 9, F, fm_M)
    fm = encode(rng, seed + 9, "rle", fm_drawn, fm_counts, (mw, mh))
    colors = (rng.integers(0, 256, (F, fm_M, 3)).astype(np.uint8) / 255.0).astype(np.float64)
    return dict(seed=seed, frames=frames, sizes=sizes, inside=inside, layout=layout, cams=[cam, dense],
                first=dict(compact=fm, mh=mh, mw=mw, M=fm_M, colors=colors), depth_erode=int(seed % 3 == 0))


def rle_stats(frames, hw):
    """what the CPU test counts of a case's run-length frames: the runs as (frame, mask, start, length) rows (int64 [R,4])"""
    rows = []
    for f, r in enumerate(frames):
        for m in range(r.shape[0]):
            for s, n in r.runs[int(r.run_off[m]):int(r.run_off[m + 1])]:
                rows.append((f, m, int(s), int(n)))
    return np.array(rows, np.int64).reshape(-1, 4)


# ---- sequences of calls on one context (route D) ------------------------------------------------------------------------------------------------
MODES = ("off", "fused", "fused-pack")
LARGE = [(150, 37), (72, 32), (1408, 376), (70, 33)]
SMALL = [(17, 16), ODD, (16, 8), (5, 7)]
NO_BOXES = dict(none=True)


def _slot(seed, slot, calib, size, M, form, erode, hint, source):
    """the narrow case of one slot of a sequence: narrow_case of seed 16 * seed + slot's draws at the given camera, mask count and form;
    ``source``: "lent" / "host" (the dense twin: uint8 masks = the form's membership), "rle" or "ids" (the compact form itself)"""
    sub = DEFAULT_SEED_BASE + (5 * seed + 3 * slot) % DEFAULT_CASES
    k = (seed + slot) % (per(form) if form != "rle" else 1)
    cs = narrow_case(sub, calib, size=size, M=M, form=form, erode=erode, element=3, hint=hint, frames=2,
                     source=(None if form == "rle" else ID_SOURCES[(seed + slot) % 3]), k=k)
    if cs["ids_source"] != "device-offset":
        cs["k"] = 0
    if size in BIG:
        assert cs["F"] <= 2 and cs["M"] <= 8
    cs["op_source"] = source
    return cs


def sequence(seed, calib):
    """The ops of a seed's sequence, 12 or 13 calls on ONE context (dicts with ``kind``):
      0  narrow  dense masks LENT from a device tensor at a large camera, 1-byte labels
      1  narrow  run-length masks at that camera, 4-byte labels (1-byte at a full-size camera: 8 masks there), one erosion; on even
                 seeds behind a pending hint of rectangles that do not hold
      2  rerun   no set-up call in order; the compact setter again in a pipelined mode
      3  wide    run_wide on an ID map (NULL corners: the boxes in force) -- another form than the narrow masks in force
      4  set_element 5
      5  rerun   in order the packed masks keep the 3 x 3 element; a pipelined rerun sets them again and erodes with the 5 x 5
      6  narrow  an ID map at a SMALL camera (label_a / label_b shrink), 2-byte labels, element 3 again, behind a pending hint
      7  narrow  the DENSE twin of 6 from host memory with no hint of its own: it must not see the hint 6 consumed
      8  label   get_label_image (a pipelined mode is switched off first and the masks are set again, as §27 does)
      9  set_pipelined  the next mode of MODES
      10 narrow  run-length masks (even seeds) or an ID map (odd seeds) at a large camera again, 1-byte labels
      11 clear_boxes, 12 rerun (even seeds: the rerun counts no box)  |  11 wide on run-length masks (odd seeds)
    The first camera is a full-size one on every fourth seed."""
    rng = np.random.default_rng([seed, 303])
    L0 = LARGE[2] if seed % 4 == 0 else LARGE[seed % 2 if seed % 4 != 3 else 3]
    L1 = LARGE[(seed + 1) % 2]
    Sm = SMALL[(seed // 2) % 4]
    idf = FORMS[1 + seed % 2]
    a = _slot(seed, 0, calib, L0, (8, 1)[seed % 2] if L0 not in BIG else 8, "rle", 0, False, "lent")
    b = _slot(seed, 1, calib, L0, (17, 31, 32)[seed % 3] if L0 not in BIG else 8, "rle", 1, seed % 2 == 0, "rle")
    c = _slot(seed, 2, calib, Sm, (9, 16)[seed % 2], idf, 0, True, "ids")
    d = dict(c, op_source="host", hint=False, rects=None, rects_mode="none")
    e_form = "rle" if seed % 2 == 0 else FORMS[2 - seed % 2]
    e = _slot(seed, 3, calib, L1, (8, 1, 3)[seed % 3], e_form, (seed // 2) % 2, False, "rle" if e_form == "rle" else "ids")

    def wide(i, cs, form):
        cam = _compact_camera(seed, i, np.random.default_rng([seed, 400 + i]), calib, cs["sizes"], (cs["W"], cs["H"]), (33, 40)[(seed + i) % 2] if (cs["W"], cs["H"]) not in BIG else 33, form)
        cam.update(ids_source=ID_SOURCES[(seed + i) % 3], k=(seed + i) % (per(form) if form != "rle" else 1))
        if cam["ids_source"] != "device-offset":
            cam["k"] = 0
        if min(cs["W"], cs["H"]) < 16:
            cam["erode"] = min(cam["erode"], 1)
        return dict(kind="wide", cam=cam)

    ops = [dict(kind="narrow", case=a), dict(kind="narrow", case=b), dict(kind="rerun"), wide(3, b, idf), dict(kind="set_element", k=5),
           dict(kind="rerun"), dict(kind="narrow", case=c), dict(kind="narrow", case=d), dict(kind="label"), dict(kind="set_pipelined"),
           dict(kind="narrow", case=e)]
    ops += [dict(kind="clear_boxes"), dict(kind="rerun")] if seed % 2 == 0 else [wide(11, e, "rle")]
    del rng
    return dict(seed=seed, ops=ops)


class Model:
    """The state include/lpf.h documents, as far as the sequences move it; apply(op) returns what the op must give.  The rules, each
    with the header's sentence:
      camera    lpf_set_camera: in force until the next one
      masks     lpf_set_masks_rle / _ids: "Afterwards the context is in the state lpf_set_masks_u8 leaves for the equivalent dense masks
                ... with the same erode_iters"; "a pending lpf_set_mask_rects hint is consumed (and ignored)": the reference is hint=False,
                and the hint is gone for the dense setter that follows
      element   lpf_set_erosion_element: "From then on every erosion of the context uses it"; "Masks already packed keep the element
                they were packed with"
      rerun     in order nothing is set again: "every later lpf_run / lpf_run_batch / lpf_run_frame (masks == NULL) gives the same
                outputs"; in a pipelined mode, and after a mode switch, the masks are set again (lpf_set_pipelined: the masks are set
                before every run of a pipelined stream) -- with the element then in force
      boxes     in force until set again or cleared; lpf_run_wide with NULL corners: "the boxes in force"
      label     lpf_get_label_image: the label image of the masks in force"""

    def __init__(self, mode="off"):
        self.mode, self.element, self.case, self.packed_with, self.boxes, self.stale = mode, 3, None, 3, None, False

    def _refs(self):
        cs = dict(self.case, element=self.packed_with)
        if self.boxes is NO_BOXES:
            cs = dict(cs, cam0=[np.zeros((0, 8, 3)) for _ in range(cs["F"])], box_source="velo-host")
        return cs, NG.reference(cs, hint=False)

    def _boxes_in_force(self, refs):
        if self.boxes is NO_BOXES:
            return dict(keep=[np.zeros(0, bool)] * len(refs), velo=[np.zeros((0, 8, 3))] * len(refs), oriented=self.case["oriented"])
        own = NG.reference(self.boxes, hint=False) if self.boxes is not self.case else refs
        return dict(keep=[r["visible"] for r in own], velo=[r["corners_velo"] for r in own], oriented=self.boxes["oriented"])

    def apply(self, op):
        kind = op["kind"]
        if kind == "narrow":
            cs = op["case"]
            self.element = 3                                      # (the op sets the element back before its masks)
            self.case, self.packed_with, self.boxes, self.stale = cs, 3, cs, False
            cs_, refs = self._refs()
            return dict(kind=kind, case=cs_, refs=refs, setup=("element", "camera", "hint" if cs["hint"] else "", "masks", "boxes"))
        if kind == "rerun":
            again = self.mode != "off" or self.stale
            if again:
                self.packed_with, self.stale = self.element, False
            cs_, refs = self._refs()
            return dict(kind=kind, case=cs_, refs=refs, setup=("masks",) if again else ())
        if kind == "wide":
            import sequence_fuzz_cases as SQ
            cs_, refs = self._refs()
            want = SQ.wide_reference(op["cam"], cs_["frames"], SQ._camera_of(cs_), self._boxes_in_force(refs), self.element)
            return dict(kind=kind, frames=cs_["frames"], refs=want, setup=())
        if kind == "set_element":
            self.element = op["k"]
            return dict(kind=kind, setup=())
        if kind == "set_pipelined":
            self.mode = MODES[(MODES.index(self.mode) + 1) % 3]
            self.stale = True
            return dict(kind=kind, mode=self.mode, setup=())
        if kind == "clear_boxes":
            self.boxes = NO_BOXES
            return dict(kind=kind, setup=())
        if kind == "label":
            setup = ()
            if self.mode != "off":
                self.mode, self.packed_with, setup = "off", self.element, ("pipelined-off", "masks")
            cs_ = dict(self.case, element=self.packed_with)
            return dict(kind=kind, case=cs_, label=NG.label_images(cs_, hint=False), setup=setup)
        raise KeyError(kind)


def expectations(seq, mode):
    """what every op of the sequence must give on a context that starts in ``mode``"""
    model = Model(mode)
    return [model.apply(op) for op in seq["ops"]]


# ---- batches for the lab build's range limits (route E) ---------------------------------------------------------------------------------------
def range_case(seed, calib):
    """A batch for lpf_depth_maps_rle / lpf_first_match_rle under the lab build's range limits: 5 to 7 frames (by the seed) of at most
    2049 points at 37 x 23 or 150 x 37, run-length masks with ragged run counts (the perturbations), ragged M and ONE frame without
    runs (frame seed % F), and colours.  In wide_case's shape: frames, cams = [the camera]."""
    F = 5 + seed % 3
    frames, sizes, inside, layout = _wide_frames(seed, calib, F)
    frames = [p[:2049] for p in frames]
    sizes = [len(p) for p in frames]
    rng = np.random.default_rng([seed, 505])
    size, M = (ODD, (150, 37))[seed % 2], (33, 65, 9)[seed % 3]
    cam = WG._draw_camera(WG.rank(seed), rng, calib, sizes, 256, size=size, M=M)
    counts = [M if f % 2 == 0 else int(rng.integers(1, M)) for f in range(F)]
    counts[seed % F] = 0
    counts[(seed + 1) % F] = M
    comp = encode(rng, seed, "rle", cam["member"], counts, size)
    cam.update(kind="u8", binarize="astype", masks=comp["member"], member=comp["member"], rects=None, rects_mode="none", compact=comp, form="rle",
               erode=0)
    colors = (rng.integers(0, 256, (F, M, 3)).astype(np.uint8) / 255.0).astype(np.float64)
    return dict(seed=seed, frames=frames, sizes=sizes, inside=inside, layout=layout, cams=[cam], colors=colors)


def check_label(got, want, what):
    """lpf_get_label_image against the reference label images, frame by frame, bit for bit"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, "get_label_image", got.shape, want.shape)
    for f in range(len(want)):
        assert np.array_equal(got[f], want[f]), (what, "get_label_image", f)


def case(seed, calib):
    """everything a seed draws for the single-call routes: dict(narrow=narrow_case, wide=wide_case); deterministic from the seed"""
    return dict(narrow=narrow_case(seed, calib), wide=wide_case(seed, calib))
