"""The narrow fuzz's case generator and checker (tests/narrow_fuzz_cases.py) on the CPU: over the default seeds of
tests/test_gpu_fuzz_narrow.py, and from the C oracle alone, the cases reach the edges they exist for -- these are conditions, so a
change to the generator that empties the fuzz fails here, without a GPU -- and the checker raises on one wrong entry of each kind."""
import copy

import numpy as np
import pytest

import narrow_fuzz_cases as G
from oracle import cpu_oracle as orc


@pytest.fixture(scope="module")
def survey(calib):
    """the default seeds' cases and their oracle results"""
    rows = []
    for seed in G.default_seeds():
        cs = G.case(seed, calib)
        rows.append((cs, G.reference(cs)))
    return rows


def _live(refs):
    """some frame has valid points and labelled ones"""
    return any(r["n_valid"] > 0 and r["n_labelled"] > 0 for r in refs)


def test_case_is_deterministic_from_the_seed(calib):
    a, b = G.case(G.DEFAULT_SEED_BASE + 1, calib), G.case(G.DEFAULT_SEED_BASE + 1, calib)
    assert a["sizes"] == b["sizes"] and a["dmax"] == b["dmax"] and a["oriented"] == b["oriented"]
    for k in ("frames", "cam0"):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k]))
    assert np.array_equal(a["masks"], b["masks"], equal_nan=True) and np.array_equal(a["rects"], b["rects"]) and np.array_equal(a["K"], b["K"])


def test_default_case_count_stays_small():
    assert G.DEFAULT_CASES <= 16 and len(G.default_seeds()) == G.DEFAULT_CASES


def test_every_listed_value_occurs(survey):
    cases = [cs for cs, _ in survey]
    assert {(cs["W"], cs["H"]) for cs in cases} == set(G.CAMERAS)
    assert {cs["dmin"] for cs in cases} == set(G.DEPTH_MIN) and {cs["dmax"] for cs in cases} == set(G.DEPTH_MAX)
    assert {cs["F"] for cs in cases} == {1, 2, 3, 4}
    assert {n for cs in cases for n in cs["sizes"]} == set(G.SIZES)
    assert {cs["M"] for cs in cases} == set(G.MASK_COUNTS)
    assert {cs["kind"] for cs in cases} == set(G.KINDS) and {cs["binarize"] for cs in cases if cs["kind"] != "u8"} == set(G.WG.RULES)
    assert {cs["erode"] for cs in cases} == set(G.ERODE)
    assert {cs["element"] for cs in cases if cs["erode"]} == set(G.ELEMENTS)
    assert all(min(cs["W"], cs["H"]) >= 16 for cs in cases if cs["element"] == 5)
    assert {cs["source"] for cs in cases} == set(G.SOURCES)
    assert {cs["rects_mode"] for cs in cases} == set(G.RECTS)
    assert {len(b) for cs in cases for b in cs["cam0"]} == set(G.BOX_COUNTS)
    assert {cs["oriented"] for cs in cases} == {False, True}
    assert {cs["box_source"] for cs in cases} == set(G.BOX_SOURCES)
    assert {cs["outs"] for cs in cases} == set(G.OUTPUT_SETS)
    assert sum(cs["want_float"] for cs in cases) * 2 == len(cases)


def test_all_five_empty_frame_layouts_occur(survey):
    seen = set()
    for cs, _ in survey:
        seen |= G.WG.empty_layouts(cs["sizes"])
    assert seen == {"first", "last", "two", "all", "single"}


def test_mask_counts_cameras_and_sources_meet_valid_and_labelled_points(survey):
    """(no masks: nothing can be labelled -- that case has valid points)"""
    live = [cs for cs, refs in survey if _live(refs)]
    assert {cs["M"] for cs in live} == set(G.MASK_COUNTS) - {0}
    assert any(cs["M"] == 0 and any(r["n_valid"] > 0 for r in refs) for cs, refs in survey)
    assert {(cs["W"], cs["H"]) for cs in live} == set(G.CAMERAS)
    assert {cs["source"] for cs in live} == set(G.SOURCES)
    assert {cs["kind"] for cs in live} == set(G.KINDS) and {cs["erode"] for cs in live} == set(G.ERODE)
    assert any(cs["erode"] and cs["element"] == 5 for cs in live)


def test_every_pack_and_label_width_is_reached(survey):
    """by shape alone (hw % 16, alignment, element): all three pack kernels, and 1-, 2- and 4-byte label images out of both the
    streaming and the tiled pack; a lent mask tensor that is not 16-byte aligned at a size that would stream; a label image handed
    over for M <= 8 (4-byte labels where the packs make 1-byte ones)"""
    live = [cs for cs, refs in survey if _live(refs)]
    kinds = {(G.pack_kind(cs), G.label_bytes(cs["M"])) for cs in live}
    assert {k for k, _ in kinds} == {"stream", "tiled", "element", None}
    assert {w for k, w in kinds if k == "stream"} == {1, 2, 4} and {w for k, w in kinds if k == "tiled"} == {1, 2, 4}
    unaligned = [cs for cs in live if cs["source"] == "lent-unaligned" and (cs["W"] * cs["H"]) % 16 == 0 and not cs["erode"]]
    assert {cs["kind"] == "u8" for cs in unaligned} == {True} and any(cs["W"] == 1408 for cs in unaligned)
    assert any(cs["source"] == "lent-unaligned" and cs["kind"] != "u8" and (cs["W"] * cs["H"]) % 16 == 0 for cs in live)
    assert any(cs["source"] == "label" and 0 < cs["M"] <= 8 for cs in live) and any(cs["source"] == "label" and cs["M"] > 16 for cs in live)


def _next_row_labelled(cs, refs):
    """labelled points whose pixel lies in the part of its 16-pixel group (of the flat image) that runs on into the next row"""
    W = cs["W"]
    n = 0
    for r in refs:
        vi = r["valid_idx"][r["label_valid"] != 0]
        o = r["v"][vi].astype(np.int64) * W + r["u"][vi]
        n += int(np.count_nonzero(r["v"][vi] > (o - o % 16) // W))
    return n


def test_a_streaming_pack_with_rectangles_straddles_rows(survey):
    """W % 16 != 0, hw % 16 == 0, W >= 16, the hint applies, the streaming pack is taken and a dense frame has it run in every launch
    form: labelled points sit in the next-row part of a group -- with rectangles that hold and with rectangles that do not"""
    hit = set()
    for cs, refs in survey:
        if cs["W"] % 16 and G.pack_kind(cs) == "stream" and G.hint_applies(cs) and _next_row_labelled(cs, refs) > 0:
            assert any(2 * n > cs["W"] * cs["H"] for n in cs["sizes"])
            hit.add(cs["rects_mode"] == "not-holding")
    assert hit == {False, True}


def test_rectangles_that_do_not_hold_bite_where_the_hint_applies_and_nowhere_else(survey):
    applies = ignored = narrow = 0
    for cs, refs in survey:
        if cs["rects_mode"] != "not-holding":
            continue
        plain = G.reference(cs, hint=False)
        same = all(np.array_equal(a["label_bits"], b["label_bits"]) for a, b in zip(refs, plain))
        if G.hint_applies(cs):
            assert not same, cs["seed"]
            applies += 1
        else:
            assert same and _live(refs), cs["seed"]
            ignored += 1
            narrow += cs["W"] < 16 and cs["kind"] == "u8" and cs["erode"] == 0          # dropped for the width alone
    assert applies and ignored >= 2 and narrow


def test_sparse_and_dense_frames_occur_with_rectangles_at_small_cameras(survey):
    sparse = dense = 0
    for cs, refs in survey:
        if G.hint_applies(cs) and (cs["W"], cs["H"]) != (1408, 376):
            for n, r in zip(cs["sizes"], refs):
                if n and r["n_labelled"]:
                    sparse += 2 * n <= cs["W"] * cs["H"]
                    dense += 2 * n > cs["W"] * cs["H"]
    assert sparse >= 2 and dense >= 2, (sparse, dense)


def test_points_on_depth_min_and_behind_the_camera(survey):
    """a placed point whose depth is depth_min exactly, inside the image and not valid, under both depth_min != 0; valid points of
    negative depth under depth_min = -5"""
    on, behind = set(), 0
    for cs, refs in survey:
        for f, r in enumerate(refs):
            at = cs["on_dmin"][f]
            if at >= 0:
                assert cs["dmin"] != 0.0 and r["depth"][at] == cs["dmin"], (cs["seed"], f)
                assert 0 <= r["u"][at] < cs["W"] and 0 <= r["v"][at] < cs["H"] and at not in r["valid_idx"], (cs["seed"], f)
                on.add(cs["dmin"])
            if cs["dmin"] < 0:
                behind += int(np.count_nonzero(r["depth"][r["valid_idx"]] < 0))
    assert on == {0.5, -5.0} and behind >= 4, (on, behind)


def test_filter_visible_drops_and_keeps(survey):
    n = 0
    for cs, refs in survey:
        if cs["box_source"] == "cam0-visible":
            n += any(0 < r["visible"].sum() < len(r["visible"]) and r["count_mb"].any() for r in refs)
        else:
            assert all(r["visible"].all() for r in refs)
    assert n >= 2


def test_most_frames_have_valid_and_labelled_points(survey):
    live = [r for cs, refs in survey if cs["M"] for n, fr, r in zip(cs["sizes"], cs["inside"], refs) if n >= 63 and fr > 0]
    good = [r for r in live if r["n_valid"] > 0 and r["n_labelled"] > 0]
    assert len(live) >= 12 and 4 * len(good) >= 3 * len(live), (len(good), len(live))


def test_tight_capacity_mixes_frames_that_fit_and_frames_that_overflow(survey):
    mixed = 0
    for cs, refs in survey:
        cap = G.tight_inst_cap(refs) if cs["tight_cap"] else None
        if cap is not None and "inst_idx" in G.fields(cs):
            over = [r["need"] > cap for r in refs]
            mixed += any(over) and not all(over)
    assert mixed >= 2


def test_a_first_strict_maximum_tie_occurs(survey):
    assert any(((r["count_mb"] == r["best_cnt"][:, None]).sum(axis=1)[r["best_cnt"] > 0] >= 2).any() for _, refs in survey for r in refs
               if r["count_mb"].size)


def test_reference_label_image_is_the_oracles(survey):
    """no rectangles, 3 x 3 element: the reference label image is orc.pack_masks of the binarised masks"""
    for cs, refs in survey:
        if cs["rects_mode"] == "none" and cs["element"] == 3 and cs["M"]:
            for f, r in enumerate(refs):
                assert np.array_equal(r["label_img"], orc.pack_masks(cs["member"][f], cs["erode"], cs["H"], cs["W"]))


# ---- the checker ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checked(survey):
    """a case with float outputs, filtered boxes, a tie-free best box and lists to corrupt; the frame to corrupt"""
    for cs, refs in survey:
        for f, r in enumerate(refs):
            if cs["want_float"] and r["n_valid"] > 1 and any(len(l) >= 2 for l in r["inst_lists"]) and r["count_mb"].any():
                return cs, refs, f
    raise AssertionError("no default seed has float outputs, lists and box counts in one frame")


def _result(refs):
    got = copy.deepcopy(refs)
    for r in got:
        for k in ("need", "label_img", "corners_velo", "inst_idx"):
            r.pop(k, None)
    return got


def test_checker_passes_the_oracle(survey):
    for cs, refs in survey:
        G.check(cs, _result(refs), refs)


def _swap_list(r):
    l = next(l for l in r["inst_lists"] if len(l) >= 2)
    l[0], l[1] = l[1], l[0]


def _other_box(r):
    m = int(np.argmax(r["best_cnt"]))
    r["best_box"][m] = (r["best_box"][m] + 1) % r["count_mb"].shape[1] if r["count_mb"].shape[1] > 1 else -1


def _flip(key, at=-1):
    def f(r):
        r[key][at] ^= 1
    return f


def _bump(key):
    def f(r):
        r[key] = r[key] + 1
    return f


def _nudge(key):
    def f(r):
        r[key][0] = np.nextafter(r[key][0], np.inf)
    return f


CORRUPTIONS = {"u": _flip("u"), "v": _flip("v"), "label_bits": lambda r: _flip("label_bits", r["valid_idx"][0])(r),
               "valid_idx": lambda r: r.update(valid_idx=r["valid_idx"][:-1]), "u_valid": _flip("u_valid"), "v_valid": _flip("v_valid"),
               "label_valid": _flip("label_valid"), "inst_lists": _swap_list, "inst_count": _flip("inst_count", 0),
               "count_mb": lambda r: r["count_mb"].__setitem__((-1, -1), r["count_mb"][-1, -1] + 1), "best_box": _other_box,
               "best_cnt": _flip("best_cnt", 0), "n_valid": _bump("n_valid"), "n_labelled": _bump("n_labelled"),
               "inst_overflow": _bump("inst_overflow"), "depth": _nudge("depth"), "uf": _nudge("uf"), "vf": _nudge("vf"),
               "visible": lambda r: r["visible"].__setitem__(0, not r["visible"][0])}


@pytest.mark.parametrize("key", sorted(CORRUPTIONS))
def test_checker_notices_one_wrong_entry(checked, key):
    cs, refs, f = checked
    got = _result(refs)
    CORRUPTIONS[key](got[f])
    with pytest.raises(AssertionError) as e:
        G.check(cs, got, refs, route="corrupted")
    assert e.value.args[0][:4] == (cs["seed"], "corrupted", f, key)


def test_checker_skips_only_the_lists_of_an_overflowing_frame(checked):
    cs, refs, f = checked
    got = _result(refs)
    got[f]["inst_overflow"] = 1
    _swap_list(got[f])
    G.check(cs, got, refs, inst_cap=refs[f]["need"] - 1)
    got[f]["inst_count"][0] += 1
    with pytest.raises(AssertionError):
        G.check(cs, got, refs, inst_cap=refs[f]["need"] - 1)
