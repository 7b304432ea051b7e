"""The wide fuzz's case generator and checker (tests/wide_fuzz_cases.py) on the CPU: over the default seeds of
tests/test_gpu_fuzz_wide.py, and from the C oracle alone, the cases reach the edges they exist for -- these are conditions, so a
change to the generator that empties the fuzz fails here, without a GPU -- and the checker raises on one wrong entry of each kind."""
import copy

import numpy as np
import pytest

import wide_fuzz_cases as G


@pytest.fixture(scope="module")
def survey(calib):
    """the default seeds' cases, reduced to what the conditions below count (single-camera cases; the oracle per frame)"""
    rows = []
    for seed in G.default_seeds():
        cs = G.case(seed, calib)
        cam = cs["cams"][0]
        refs = G.reference(cs)
        frames = []
        for f, r in enumerate(refs):
            words = r["label_valid_words"]
            masked = words[words.any(axis=1)] if cam["M"] else words[:0]
            cm, bc = r["count_mb"], r["best_cnt"]
            frames.append(dict(N=cs["sizes"][f], inside=cs["inside"][f], B=len(cam["boxes"][f]), n_valid=r["n_valid"], n_labelled=r["n_labelled"],
                               n_masked=len(masked), every_word=bool(len(masked)) and bool(masked.any(axis=0).all()),
                               tie=bool(((cm == bc[:, None]).sum(axis=1)[bc > 0] >= 2).any()) if cm.size else False,
                               need=int(r["inst_count"].sum()),
                               direct=G.expects_direct(cam, f, cs["sizes"][f], True)))
        rows.append(dict(seed=seed, sizes=cs["sizes"], M=cam["M"], size=(cam["W"], cam["H"]), F=cam["F"], kind=cam["kind"], erode=cam["erode"],
                         rects=cam["rects_mode"], fw=cam["fw_mode"], binarize=cam["binarize"], frames=frames))
    return rows


def test_case_is_deterministic_from_the_seed(calib):
    a, b = G.case(G.DEFAULT_SEED_BASE + 2, calib, n_cams=2), G.case(G.DEFAULT_SEED_BASE + 2, calib, n_cams=2)
    assert a["sizes"] == b["sizes"]
    for x, y in zip(a["frames"], b["frames"]):
        assert np.array_equal(x, y)
    for ca, cb in zip(a["cams"], b["cams"]):
        assert np.array_equal(ca["masks"], cb["masks"], equal_nan=True) and np.array_equal(ca["K"], cb["K"])
        assert all(np.array_equal(p, q) for p, q in zip(ca["boxes"], cb["boxes"]))


def test_every_listed_value_occurs(survey):
    assert {n for r in survey for n in r["sizes"][:r["F"]]} == set(G.SIZES)
    assert {r["M"] for r in survey} == set(G.MASK_COUNTS)
    assert {r["M"] for r in survey if any(fr["n_valid"] > 0 for fr in r["frames"])} == set(G.MASK_COUNTS)      # ... and with valid points
    assert {fr["B"] for r in survey for fr in r["frames"]} == set(G.BOX_COUNTS)
    assert {r["size"] for r in survey} == set(G.CAMERAS)
    assert {r["kind"] for r in survey} == {"u8", "f32"} and {r["erode"] for r in survey} == {0, 1, 2}
    assert {r["rects"] for r in survey} == {"none", "tight", "sentinel"} and {r["fw"] for r in survey} == {"tight", "sentinel"}
    assert {r["binarize"] for r in survey if r["kind"] == "f32"} == set(G.RULES)


def test_all_five_empty_frame_layouts_occur(survey):
    seen = set()
    for r in survey:
        seen |= G.empty_layouts(r["sizes"][:r["F"]])
    assert seen == {"first", "last", "two", "all", "single"}


def test_dense_and_short_masked_lists_occur(survey):
    assert any(fr["n_masked"] > 4096 and fr["every_word"] for r in survey if r["M"] >= 65 for fr in r["frames"])
    assert any(0 < fr["n_masked"] < 8 for r in survey for fr in r["frames"])           # box-count parts with lo >= hi
    assert any(fr["n_masked"] < 8 and fr["N"] > 0 for r in survey if r["M"] for fr in r["frames"])


def test_masked_points_are_a_proper_part_of_the_valid_ones_somewhere(survey):
    """more than one label word and 0 < n_labelled < n_valid: the scan's two carries and the masked list's compaction differ"""
    assert any(0 < fr["n_labelled"] < fr["n_valid"] and fr["n_valid"] > 256 for r in survey if r["M"] >= 33 for fr in r["frames"])


@pytest.mark.parametrize("max_masks", [32, 256])
def test_multi_camera_cases_keep_their_frames(max_masks):
    """The run_cams (up to 32 masks) and run_cams_wide cases of the default seeds, by their shapes alone: among the cases of two or
    more cameras, one with masks runs three frames or more with an empty frame among them; every mask count of the short list occurs
    with several cameras; run_cams_wide sees a camera of 1..32 masks next to a wider one."""
    ragged, mixed, counts = 0, 0, set()
    for seed in G.default_seeds():
        sizes, cams = G.case_shapes(seed, 1 + seed % 4, max_masks)
        F = min(c[3] for c in cams)
        Ms = [c[2] for c in cams]
        if len(cams) >= 2:
            counts |= set(Ms)
            ragged += F >= 3 and max(Ms) > 0 and 0 in sizes[:F] and any(sizes[:F])
            mixed += any(0 < m <= 32 for m in Ms) and any(m > 32 for m in Ms)
    assert ragged >= 2, ragged
    if max_masks == 32:
        assert counts == {0, 1, 31, 32}
    else:
        assert mixed >= 2, mixed


def test_most_frames_have_valid_and_labelled_points(survey):
    live = [fr for r in survey for fr in r["frames"] if fr["N"] >= 63 and fr["inside"] > 0]
    good = [fr for fr in live if fr["n_valid"] > 0 and fr["n_labelled"] > 0]
    assert len(live) >= 12 and 4 * len(good) >= 3 * len(live), (len(good), len(live))


def test_a_first_strict_maximum_tie_occurs(survey):
    assert any(fr["tie"] for r in survey for fr in r["frames"])


def test_overflow_mixes_and_both_frame_wide_forms_occur(survey):
    """the odd seeds' tight inst_cap leaves frames that fit next to frames that overflow; lpf_run_frame_wide's routing rule sends
    frames of the default seeds both ways"""
    mixed = 0
    for r in survey:
        needs = [fr["need"] for fr in r["frames"]]
        if r["seed"] % 2 and max(needs) >= 2 and len(needs) > 1 and min(needs) < max(needs):
            mixed += 1
    assert mixed >= 2
    direct = [fr["direct"] for r in survey for fr in r["frames"] if fr["N"]]
    assert any(direct) and not all(direct)


def test_direct_case_is_what_it_says(calib):
    """the deterministic case of the direct form: every frame takes it, chunk 0 of the last frame has no valid point, the candidates
    sit in the last label word only and are no multiple of four there, and the rectangles that do not hold change the result"""
    for M in (32, 33, 48):
        cs = G.direct_case(M, calib)
        cam = cs["cams"][0]
        refs = G.reference(cs)
        assert all(G.expects_direct(cam, f, n, True) for f, n in enumerate(cs["sizes"]))
        assert refs[5]["n_valid"] > 0 and refs[5]["valid_idx"].min() >= 1024
        live = cam["member"][0].any(axis=(1, 2))
        first = 32 * ((M + 31) // 32 - 1)
        assert not live[:first].any() and live[first:].sum() % 4 != 0
        assert all(r["n_labelled"] > 0 for r in refs[1:]) and refs[4]["n_labelled"] > 4096
        zeroed = G.zeroed_outside(cam, "not-holding", 4)
        assert G.oracle_result(cam, cs["frames"][4], 4, member=zeroed)["n_labelled"] not in (0, refs[4]["n_labelled"])


# ---- the checker ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checked(calib, survey):
    """a case with more than 32 masks, a tie and lists to corrupt; its oracle result and where the tie is"""
    for r in survey:
        if r["M"] > 32 and any(fr["tie"] and fr["n_valid"] > 1 for fr in r["frames"]):
            cs = G.case(r["seed"], calib)
            refs = G.reference(cs)
            f = next(i for i, fr in enumerate(r["frames"]) if fr["tie"] and fr["n_valid"] > 1)
            return cs, refs, f
    raise AssertionError("no default seed has more than 32 masks and a tie")


def _result(refs):
    return copy.deepcopy(refs)


def test_checker_passes_the_oracle(checked):
    cs, refs, _ = checked
    G.check_wide(cs["cams"][0], cs["frames"], _result(refs), refs)


def _raises(cs, refs, res):
    """both halves of the checker notice it: _check with its own run of the oracle, and the comparison with the shared reference"""
    cam = cs["cams"][0]
    with pytest.raises(AssertionError):
        G._check(cam, res, cs["frames"][:cam["F"]], list(cam["member"]), cam["erode"], cam["boxes"], cam["oriented"], dmin=cam["dmin"], dmax=cam["dmax"])
    with pytest.raises(AssertionError):
        G.check_wide(cam, cs["frames"], res, refs, fresh=False)


def test_checker_notices_two_list_entries_swapped(checked):
    cs, refs, f = checked
    res = _result(refs)
    m = next(i for i, l in enumerate(res[f]["inst_lists"]) if len(l) >= 2)
    l = res[f]["inst_lists"][m]
    l[0], l[1] = l[1], l[0]
    _raises(cs, refs, res)


def test_checker_notices_one_bit_of_the_last_label_word(checked):
    cs, refs, f = checked
    res = _result(refs)
    M = cs["cams"][0]["M"]
    res[f]["label_words"][res[f]["valid_idx"][0], -1] ^= np.uint32(1) << np.uint32((M - 1) % 32)
    _raises(cs, refs, res)


def test_checker_notices_the_other_box_of_a_tie(checked):
    cs, refs, f = checked
    res = _result(refs)
    cm, bc = res[f]["count_mb"], res[f]["best_cnt"]
    m = next(i for i in range(len(bc)) if bc[i] > 0 and (cm[i] == bc[i]).sum() >= 2)
    other = np.flatnonzero(cm[m] == bc[m])[1]
    assert other != res[f]["best_box"][m]
    res[f]["best_box"][m] = other
    _raises(cs, refs, res)


def test_checker_notices_one_count(checked):
    cs, refs, f = checked
    res = _result(refs)
    res[f]["count_mb"][-1, -1] += 1
    _raises(cs, refs, res)


def test_checker_notices_a_dropped_valid_index(checked):
    cs, refs, f = checked
    res = _result(refs)
    res[f]["valid_idx"] = res[f]["valid_idx"][:-1]
    _raises(cs, refs, res)
