"""Seeded differential fuzz of the wide and multi-camera passes -- lpf_run_wide, lpf_run_frame_wide (direct form and pack),
lpf_run_cams, lpf_run_cams_wide, lpf_depth_maps -- against the C oracle run once per group of 32 masks on the binarised masks eroded
by the oracle, bit for bit in every compared array.  The cases come from tests/wide_fuzz_cases.py: image sizes that are no multiple
of the pack's 64 x 16 tile, frame sizes around the 1024-point chunk and its four points per thread, every layout of empty frames, mask
counts around the label word and the direct form's limit, full and random masks in every word (dense lists), box counts around the
64-box word that differ per frame, float masks with odd values, erosion, rectangles with "no limit" entries.  What the default seeds
reach is asserted on the CPU (tests/test_wide_fuzz_cases.py).  LPF_FUZZ_CASES and LPF_FUZZ_SEED_BASE choose other seeds, as in
tests/test_gpu_fuzz.py; test_ladder_in_one_batch is the one deterministic case, and the only one above 20 000 points per frame."""
import numpy as np
import pytest

import wide_fuzz_cases as G
from lidar_object_detection_amd._native import LpfContext
from oracle import cpu_oracle as orc
from test_gpu_depth_maps import _expect, _same
from test_gpu_frame_wide import _host, _outs

pytestmark = pytest.mark.gpu

SEEDS = G.seeds()


class _Fuzz:
    """one seed's case -- 1 + seed % 4 cameras of up to 256 masks; camera 0 alone is the single-camera case -- and its oracle
    results, computed when first asked for and shared by the tests of the seed"""

    def __init__(self, seed, calib):
        self.seed = seed
        self.cs = G.case(seed, calib, n_cams=1 + seed % 4)
        self._refs = {}

    def refs(self, k=0):
        if k not in self._refs:
            self._refs[k] = G.reference(self.cs, k)
        return self._refs[k]


@pytest.fixture(scope="module", params=SEEDS)
def fuzz(request, calib):
    """(module scope: pytest runs the tests seed by seed, and a case lives only as long as its seed's tests)"""
    return _Fuzz(request.param, calib)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _masks_where(cam, F, device):
    """the camera's masks and rectangles of the first F frames, in host memory or as GPU tensors"""
    masks = cam["masks"][:F]
    rects = cam["rects"][:F] if cam["rects"] is not None else None
    if device:
        return _dev(masks), (_dev(rects) if rects is not None else None)
    return masks, rects


def _context(cam, F=None):
    ctx = LpfContext(0)
    ctx.set_camera(cam["T"], cam["K"], cam["W"], cam["H"], cam["dmin"], cam["dmax"])
    if F is not None:
        ctx.set_boxes(cam["boxes"][:F], oriented=cam["oriented"])
    return ctx


def _count_launches(ctx):
    """how often the binding wires a wide run's host outputs: once per native call"""
    calls = []
    orig = ctx._wide_host_outputs

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)
    ctx._wide_host_outputs = counted
    return calls


def test_fuzz_run_wide(fuzz):
    """Host masks and device masks, float outputs and the compact valid arrays.  Odd seeds: an inst_cap below the largest frame's
    need, at which the frames that need no more fit and the others overflow -- the binding runs once more with the exact capacity."""
    seed, cs = fuzz.seed, fuzz.cs
    cam = cs["cams"][0]
    F = cam["F"]
    refs = fuzz.refs()
    cap = G.tight_inst_cap(refs) if seed % 2 else None
    with _context(cam, F) as ctx:
        calls = _count_launches(ctx)
        for device in (False, True):
            masks, rects = _masks_where(cam, F, device)
            del calls[:]
            res = ctx.run_wide(cs["frames"][:F], masks, erode_iters=cam["erode"], binarize=cam["binarize"], rects=rects, want_float=True,
                               want_valid_uv=True, inst_cap=cap)
            G.check_wide(cam, cs["frames"], res, refs, what=(seed, "device" if device else "host"), fresh=not device)
            if cap is not None:
                assert len(calls) == 2, (seed, cap, G.list_needs(refs))          # overflow, then the exact capacity


def _frame_wide_result(h, M, B):
    """lpf_run_frame_wide's device outputs (read back) as one frame's dict in run_wide's shape"""
    nv = int(h["n_valid"][0])
    io = h["inst_off"]
    return dict(u=h["uv"][:, 0], v=h["uv"][:, 1], depth=h["depth"], uf=h["u_f"], vf=h["v_f"], label_words=h["label_words"].view(np.uint32),
                valid_idx=h["valid_idx"][:nv], count_mb=h["count_mb"].reshape(M, B), best_box=h["best_box"], best_cnt=h["best_cnt"],
                inst_count=h["inst_count"], n_valid=nv, n_labelled=int(h["n_labelled"][0]),
                inst_lists=[h["inst_idx"][io[m]:io[m + 1]] for m in range(M)], label_valid_words=h["label_valid_words"][:nv].view(np.uint32),
                u_valid=h["uv_valid"][:nv, 0], v_valid=h["uv_valid"][:nv, 1])


def _frame_wide(ctx, cam, pts, f, plain, what):
    """Frame f through make_frame_step_wide (uint8 device masks, no erosion), once per set of lpf_run_frame_wide's rectangles the
    camera has and once without; plain: the oracle's result for the masks as they are.  Rectangles that do not hold are compared
    against the masks zeroed outside them.  Which form ran is read from the context's statistics and has to be the routing
    rule's.  Returns the forms taken (True: direct)."""
    M, mem, cor = cam["M"], cam["member"][f], cam["boxes"][f]
    one = dict(cam, boxes=[cor], erode=0)
    ctx.set_boxes([cor], oriented=cam["oriented"])                            # the boxes in force: the jobs bring none
    dp, dm = _dev(pts), _dev(mem)
    seen = set()
    for which in list(cam["fw_rects"]) + [None]:
        rects = cam["fw_rects"][which][f] if which else None
        member, ref = mem, plain
        if which == "not-holding" and M:
            member = G.zeroed_outside(cam, which, f)
            ref = G.oracle_result(one, pts, 0, member=member)
        cap = max(int(ref["inst_count"].sum()), 1)
        o = _outs(len(pts), M, len(cor), cap)
        dr = _dev(rects) if rects is not None else None
        step = ctx.make_frame_step_wide(dp, dm, mask_rects=dr, inst_cap=cap, **o)
        before = ctx.stats()["wide_direct_frames"]
        step()
        ctx.sync()
        direct = ctx.stats()["wide_direct_frames"] - before
        assert direct == int(G.expects_direct(cam, f, len(pts), which is not None)), (what, f, which)
        seen.add(bool(direct))
        h = _host(o)
        assert h["inst_overflow"][0] == 0, (what, f, which)
        G.check_wide(one, [pts], [_frame_wide_result(h, M, len(cor))], [ref], member=[member],
                     what=(what, f, which, "direct" if direct else "pack"), fresh=which in ("hold", "not-holding"))
    return seen


def test_fuzz_frame_wide(fuzz):
    """Every frame of the case through make_frame_step_wide with rectangles that hold (tight, or with "no limit" entries), with
    rectangles that do not, and without.  (That the default seeds send frames both ways is asserted on the CPU.)"""
    seed, cs = fuzz.seed, fuzz.cs
    cam = cs["cams"][0]
    with _context(cam) as ctx:
        for f in range(cam["F"]):
            pts = cs["frames"][f]
            plain = fuzz.refs()[f] if cam["erode"] == 0 else G.oracle_result(dict(cam, erode=0), pts, f)
            _frame_wide(ctx, cam, pts, f, plain, seed)


@pytest.mark.parametrize("M", [32, 33, 48])
def test_direct_form_edges(M, calib):
    """The direct form of lpf_run_frame_wide at 32, 33 and 48 masks on a 333 x 141 image (wide_fuzz_cases.direct_case): a chunk
    without a valid point, candidates only in the second label word, a word whose candidates are no multiple of four, rectangles
    that hold, "no limit" rectangles on a 20 000-point frame and rectangles that do not hold.  Every frame with rectangles takes the
    direct form, the run without them the pack."""
    cs = G.direct_case(M, calib)
    cam = cs["cams"][0]
    refs = G.reference(cs)
    with _context(cam) as ctx:
        for f, pts in enumerate(cs["frames"]):
            assert _frame_wide(ctx, cam, pts, f, refs[f], "direct M=%d" % M) == {True, False}


def _cams_case(seed, cs, refs_of):
    """The case's cameras -- their own image size, masks, boxes and depth window over the same frames (as many as every camera's
    masks fit) -- as run_cams / run_cams_wide camera dicts, and every camera's oracle results"""
    F = G.common_frames(cs)
    specs, refs = [], []
    for k, cam in enumerate(cs["cams"]):
        masks, rects = _masks_where(cam, F, device=(seed + k) % 2 == 1)
        specs.append(dict(T_velo_to_rect=cam["T"], K=cam["K"], width=cam["W"], height=cam["H"], depth_min=cam["dmin"], depth_max=cam["dmax"],
                          masks=masks, rects=rects, binarize=cam["binarize"], erode_iters=cam["erode"], boxes=cam["boxes"][:F],
                          oriented=cam["oriented"]))
        refs.append(refs_of(k)[:F])
    return F, specs, refs


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz_run_cams(seed, calib):
    """C = 1 + seed % 4 cameras of up to 32 masks (their own draw): every camera of the one pass against the oracle"""
    cs = G.case(seed, calib, n_cams=1 + seed % 4, max_masks=32)
    F, specs, refs = _cams_case(seed, cs, lambda k: G.reference(cs, k))
    with LpfContext(0) as ctx:
        got = ctx.run_cams(cs["frames"][:F], specs, want_float=True, want_valid_uv=True)
    assert len(got) == len(specs)
    for k in range(len(specs)):
        assert len(got[k]) == F
        for f in range(F):
            G.compare_narrow(got[k][f], refs[k][f], (seed, "camera %d" % k, f))


def test_fuzz_run_cams_wide(fuzz):
    """C = 1 + seed % 4 cameras of up to 256 masks, cameras of up to 32 masks next to cameras of more: every camera against the
    oracle"""
    seed, cs = fuzz.seed, fuzz.cs
    F, specs, refs = _cams_case(seed, cs, fuzz.refs)
    with LpfContext(0) as ctx:
        got = ctx.run_cams_wide(cs["frames"][:F], specs, want_float=True, want_valid_uv=True)
    assert len(got) == len(specs)
    for k, cam in enumerate(cs["cams"]):
        G.check_wide(cam, cs["frames"], got[k], refs[k], what=(seed, "camera %d" % k), fresh=k > 0)    # (camera 0: test_fuzz_run_wide's)


def test_fuzz_depth_maps(fuzz):
    """The same cases through lpf_depth_maps: car m is flatnonzero(where(member_m, D, 0)) with D the oracle's last-writer depth image
    and member_m the oracle's eroded mask -- with the default capacity (host masks) and with a capacity of one entry, which every
    frame with two entries overflows (device masks)."""
    seed, cs = fuzz.seed, fuzz.cs
    cam = cs["cams"][0]
    F = cam["F"]
    want = []
    for f in range(F):
        D, win = orc.depth_image(cs["frames"][f], cam["T"], cam["K"], cam["W"], cam["H"], cam["dmin"], cam["dmax"])
        want.append(_expect(D, win, G.eroded_member(cam, f)))
    need = max(sum(len(p) for p, _, _ in cars) for cars in want)
    with _context(cam) as ctx:
        launches = []
        pinned = ctx._pinned
        ctx._pinned = lambda name, *a: (launches.append(name) if name == "dm_pix" else None, pinned(name, *a))[1]
        for cap, device in ((None, False), (1, True)):
            masks, rects = _masks_where(cam, F, device)
            del launches[:]
            got = ctx.depth_maps(cs["frames"][:F], masks, binarize=cam["binarize"], rects=rects, erode_iters=cam["erode"], cap=cap)
            assert len(got) == F
            for f in range(F):
                _same(got[f], want[f], (seed, cap, f))
            if cap == 1:
                assert len(launches) == (2 if need > 1 else 1), (seed, need)      # overflow, then the exact capacity


def test_ladder_in_one_batch(calib):
    """One batch of 0, 1, 3, 4, 5, 1023, 1024, 1025, 0, 0, 4097, 262145 and 0 points (90 % inside the image): the tails of the
    four-points-per-thread chunk, chunks that end on and one past 1024, empty frames first, last and two in a row, and the smallest
    frame whose 257 chunks take the second trip of the chunk scan.  65 masks (a third label word of one mask) mixing full, random and
    rectangle masks, box counts 0, 1, 7, 64, 65, 130 in turn.  Through run_wide and, with a second camera, run_cams_wide."""
    cs = G.ladder(calib, [(150, 37), (70, 33)])
    frames = cs["frames"]
    refs = [G.reference(cs, k) for k in range(2)]
    assert [len(p) for p in frames] == G.LADDER_SIZES and refs[0][11]["n_labelled"] > 4096
    assert all(cam["M"] == 65 for cam in cs["cams"])
    cam = cs["cams"][0]
    with _context(cam, len(frames)) as ctx:
        res = ctx.run_wide(frames, cam["masks"], erode_iters=cam["erode"], binarize=cam["binarize"], rects=cam["rects"], want_float=True,
                           want_valid_uv=True)
        G.check_wide(cam, frames, res, refs[0], what="ladder run_wide")
    specs = [dict(T_velo_to_rect=c["T"], K=c["K"], width=c["W"], height=c["H"], depth_min=c["dmin"], depth_max=c["dmax"], masks=c["masks"],
                  rects=c["rects"], binarize=c["binarize"], erode_iters=c["erode"], boxes=c["boxes"], oriented=c["oriented"]) for c in cs["cams"]]
    with LpfContext(0) as ctx:
        got = ctx.run_cams_wide(frames, specs, want_float=True, want_valid_uv=True)
    for k, c in enumerate(cs["cams"]):
        G.check_wide(c, frames, got[k], refs[k], what="ladder run_cams_wide camera %d" % k, fresh=k > 0)
