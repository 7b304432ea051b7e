"""What the default seeds of the sequence fuzz (tests/sequence_fuzz_cases.py, run on the GPU by tests/test_gpu_sequence_fuzz.py) reach,
asserted from the model and the references alone; that the checker reports one wrong entry, and one overwritten poison byte, of the
outputs it reads; that a sequence's expectations do not depend on who computes them.  No GPU."""
import hashlib

import numpy as np
import pytest

import narrow_fuzz_cases as NG
import sequence_fuzz_cases as G
from conftest import load_calib


@pytest.fixture(scope="module")
def seqs():
    cal = load_calib()
    return [G.sequence(s, cal) for s in G.default_seeds()]


@pytest.fixture(scope="module")
def exps(seqs):
    """(sequence, mode) -> expectations"""
    return {(q.seed, m): G.expectations(q, m) for q in seqs for m in G.MODES}


def _masks_of(op, e):
    """the mask count an op brings to the context, or None"""
    if op["kind"] in ("narrow", "rerun", "rerun-unset"):
        return e["case"]["M"]
    if op["kind"] in ("wide", "depth_maps"):
        return op["cam"]["M"]
    if op["kind"] == "first_match":
        return op["masks"].shape[1]
    if op["kind"] == "cams":
        return max(c["M"] for c in op["case"]["cams"])
    return None


def _all_masks(op):
    """every mask array an op hands to the context"""
    if op["kind"] == "narrow":
        return [op["case"]["masks"]]
    if op["kind"] in ("wide", "depth_maps", "depth_overlays"):
        return [np.asarray(op["cam"]["masks"])]
    if op["kind"] == "frame_wide":
        return [np.asarray(op["cam"]["member"])]
    if op["kind"] == "cams":
        return [np.asarray(c["masks"]) for c in op["case"]["cams"]]
    if op["kind"] == "first_match":
        return [op["masks"]]
    return []


def test_default_seeds_and_lengths(seqs):
    assert len(seqs) == 16 and all(10 <= len(q.ops) <= 14 for q in seqs)
    again = G.sequence(seqs[3].seed, load_calib())
    assert again.kinds() == seqs[3].kinds()


def test_every_family_and_route_is_reached(seqs):
    kinds = {k for q in seqs for k in q.kinds()}
    assert kinds == set(G.FAMILIES)
    routes = {op["route"] for q in seqs for op in q.ops if op["kind"] == "narrow"}
    assert routes == {"device", "host", "step"}
    calls = {op["call"] for q in seqs for op in q.ops if op["kind"] == "pairs"}
    assert calls == set(G.PAIR_CALLS)
    assert {op["wide"] for q in seqs for op in q.ops if op["kind"] == "cams"} == {False, True}
    sources = {op["case"]["source"] for q in seqs for op in q.ops if op["kind"] == "narrow"}
    assert sources == set(NG.SOURCES)
    boxes = {op["case"]["box_source"] for q in seqs for op in q.ops if op["kind"] == "narrow"}
    assert boxes == set(NG.BOX_SOURCES)
    for kind in ("wide", "first_match", "depth_maps", "box_views", "inside_masks", "box_points", "operators"):                # operands in host and in device memory
        assert {op["device"] for q in seqs for op in q.ops if op["kind"] == kind} == {False, True}, kind
    assert {op["place"] for q in seqs for op in q.ops if op["kind"] == "pairs"} == {"hh", "dd"}


def test_no_op_is_dropped_and_every_pass_is_followed_by_a_rerun(seqs, exps):
    """every op of a sequence has an expectation under every mode (none is dropped because it "does not fit"), and directly behind
    every wide, multi-camera and analysis call comes a rerun that rests on sticky state: in order it makes no set-up call at all"""
    followed = set()
    for q in seqs:
        for m in G.MODES:
            ex = exps[q.seed, m]
            assert len(ex) == len(q.ops) and all(e["kind"] == op["kind"] for e, op in zip(ex, q.ops))
        ex = exps[q.seed, "off"]
        for i, op in enumerate(q.ops):
            if op["kind"] in G.PASSES:
                assert q.ops[i + 1]["kind"] == "rerun", (q.seed, i)
                name = op.get("call") or (("cams-wide" if op["wide"] else "cams") if op["kind"] == "cams" else op["kind"])
                if any(exps[q.seed, m][i + 1]["setup"] == () for m in G.MODES):      # (in order under some starting mode)
                    followed.add(name)
    assert followed == {"wide", "cams", "cams-wide", "first_match", "depth_maps", "box_views", "inside_masks", "box_points", "operators", "frame_wide", "depth_overlays",
                        "clear_boxes"} | set(G.PAIR_CALLS)
    for m in ("fused", "fused-pack"):                         # in a pipelined mode: the masks again, never the boxes
        for q in seqs:
            for op, e in zip(q.ops, exps[q.seed, m]):
                if op["kind"] == "rerun":
                    assert "boxes" not in e["setup"] and "camera" not in e["setup"]


def test_cameras_shrink_and_grow(seqs):
    for q in seqs:
        area = [op["case"]["W"] * op["case"]["H"] for op in q.ops if op["kind"] == "narrow"]
        assert len(area) == 3 and area[1] < area[0] < area[2], (q.seed, area)       # large -> small -> larger: scratch reused, then grown
        # what is bounded at the full-size cameras: ONE set_camera goes there, it is the last narrow case, with at most 8 masks and
        # 2 frames; the ops behind it (pass, reruns, tail) run at that size too, the pass with 33 masks at the most
        big = [i for i, op in enumerate(q.ops) if op["kind"] == "narrow" and (op["case"]["W"], op["case"]["H"]) in G.BIG]
        assert len(big) <= 1
        for i in big:
            assert q.ops[i]["case"]["M"] <= 8 and q.ops[i]["case"]["F"] <= 2
            assert not any(op["kind"] == "narrow" for op in q.ops[i + 1:])
            for op in q.ops[i + 1:]:
                assert all(m.shape[-3] <= 33 for m in _all_masks(op) if m.shape[-2:] == q.ops[i]["case"]["masks"].shape[-2:]), (q.seed, op["kind"])
        assert sum(m.size for op in q.ops for m in _all_masks(op)) <= NG.MASK_BYTES, q.seed          # every mask an op brings, as uint8 bytes
    sizes = {(op["case"]["W"], op["case"]["H"]) for q in seqs for op in q.ops if op["kind"] == "narrow"}
    assert set(G.BIG) <= sizes and len(sizes) >= 6
    pts = [n for q in seqs for op in q.ops if op["kind"] == "narrow" for n in op["case"]["sizes"]]
    assert min(pts) == 0 and max(pts) == 20000
    assert {op["case"]["F"] for q in seqs for op in q.ops if op["kind"] == "narrow"} >= {1, 2, 3, 4}


def test_mask_counts_cross_32_down_and_up(seqs, exps):
    down = up = word = 0
    for q in seqs:
        ms = [m for m in (_masks_of(op, e) for op, e in zip(q.ops, exps[q.seed, "off"])) if m is not None]
        for a, b in zip(ms, ms[1:]):
            down += a > 32 >= b
            up += a <= 32 < b
            word += (a - 1) // 32 != (b - 1) // 32
    assert down >= 8 and up >= 8 and word >= 16, (down, up, word)
    counts = {m for q in seqs for op, e in zip(q.ops, exps[q.seed, "off"]) for m in [_masks_of(op, e)] if m is not None}
    assert {0, 1, 32, 33, 256} <= counts


def test_mode_switches_with_work_owed_and_the_refusal(seqs, exps):
    owed = {m: 0 for m in G.MODES}
    refused = plain = label_switch = no_sync = 0
    for q in seqs:
        no_sync += "sync" not in q.kinds()
        for m in G.MODES:
            for op, e in zip(q.ops, exps[q.seed, m]):
                if op["kind"] == "set_pipelined" and e["owed"]:
                    owed[m] += 1
                if op["kind"] == "rerun-unset":
                    refused += e["refuse"] == G.REFUSAL
                    plain += e["refuse"] is None
                if op["kind"] == "label" and "pipelined-off" in e["setup"]:
                    label_switch += 1
    assert owed["fused"] >= 4 and owed["fused-pack"] >= 4 and owed["off"] == 0     # (from "off" nothing is owed when the switch comes)
    assert refused >= 4 and plain >= 2 and label_switch >= 4 and no_sync >= 8
    modes = {e["mode"] for q in seqs for m in G.MODES for e in exps[q.seed, m] if e["kind"] == "set_pipelined"}
    assert modes == set(G.MODES)
    for q in seqs:                                            # the op behind a refusal is a full narrow case: it has to be right
        for i, k in enumerate(q.kinds()):
            if k == "rerun-unset":
                assert q.ops[i + 1]["kind"] == "narrow"


def test_element_change_between_a_pack_and_its_rerun(seqs, exps):
    """in order the rerun keeps the element its masks were packed with; in a pipelined mode the masks are set again and take the new
    one -- and the two references differ for a case with erosion"""
    kept = taken = differ = 0
    for q in seqs:
        for i, op in enumerate(q.ops):
            if op["kind"] != "set_element":
                continue
            assert q.ops[i + 1]["kind"] == "rerun"
            off, fused = exps[q.seed, "off"][i + 1], exps[q.seed, "fused"][i + 1]
            assert off["setup"] == () and fused["setup"] == ("masks",)
            assert off["case"]["element"] == 3 and fused["case"]["element"] == op["k"] == 5
            kept += 1
            taken += 1
            if off["case"]["erode"] and off["case"]["M"]:
                differ += any(not np.array_equal(a["label_img"], b["label_img"]) for a, b in zip(off["refs"], fused["refs"]))
    assert kept >= 8 and differ >= 2, (kept, differ)
    wide_with_5 = sum(1 for q in seqs for i, op in enumerate(q.ops) if op["kind"] in ("wide", "depth_maps", "cams") and "set_element" in q.kinds()[:i]
                      and any(c["erode"] for c in (op["case"]["cams"] if op["kind"] == "cams" else [op["cam"]])))
    assert wide_with_5 >= 2                                   # the element in force reaches the passes that erode


def _digest(x):
    h = hashlib.sha256()

    def walk(v):
        if isinstance(v, dict):
            for k in sorted(v, key=str):
                h.update(str(k).encode())
                walk(v[k])
        elif isinstance(v, (list, tuple)):
            for a in v:
                walk(a)
        elif isinstance(v, np.ndarray):
            h.update(str(v.dtype).encode() + str(v.shape).encode() + np.ascontiguousarray(v).tobytes())
        else:
            h.update(repr(v).encode())
    walk(x)
    return h.hexdigest()


def test_replaying_the_ops_on_fresh_models_gives_the_same_references(seqs, exps):
    """a fresh model fed the ops one by one gives, op for op, the references of the sequence's own model, and computing them changes
    nothing in the ops (the GPU tests share both)"""
    for q in seqs[:6]:
        before = _digest(q.ops)
        for m in G.MODES:
            model = G.Model(m)
            for i, op in enumerate(q.ops):
                assert _digest(model.apply(op)) == _digest(exps[q.seed, m][i]), (q.seed, m, i, op["kind"])
        assert _digest(q.ops) == before


def _narrow_case(seqs, exps, want_lists=True):
    for q in seqs:
        for op, e in zip(q.ops, exps[q.seed, "off"]):
            if op["kind"] == "narrow" and set(NG.fields(e["case"])) >= set(NG.ALL_FIELDS) and e["case"]["want_float"] and e["case"]["M"] > 1 and \
                    all(r["n_valid"] > 4 and r["need"] > 0 for r in e["refs"]) and any(len(c) for c in e["case"]["cam0"]):
                return e["case"], e["refs"]
    raise AssertionError("no default seed has a narrow case with every output")


def test_checker_reports_one_wrong_entry_and_one_poison_byte_of_every_narrow_output(seqs, exps):
    cs, refs = _narrow_case(seqs, exps)
    fl = NG.fields(cs)
    cap = max(r["need"] for r in refs) + 3
    good = G.forge_narrow(cs, refs, fl, cap)
    G.check_narrow(cs, good, refs, cap, "forged")
    nv, need = refs[0]["n_valid"], refs[0]["need"]
    n0 = cs["sizes"][0]
    for k in fl:                                              # one wrong entry of each output
        bad = {n: a.copy() for n, a in good.items()}
        flat = bad[k].reshape(-1).view(np.uint8)
        flat[0] ^= 1
        with pytest.raises(AssertionError):
            G.check_narrow(cs, bad, refs, cap, "one wrong entry of " + k)
    bad = {n: a.copy() for n, a in good.items()}
    bad["summary"][0] ^= 1                                    # (n_valid of frame 0)
    with pytest.raises(AssertionError):
        G.check_narrow(cs, bad, refs, cap, "a wrong summary")
    assert nv < n0, "frame 0 has room behind its valid points"
    for k, at in (("valid_idx", nv), ("uv_valid", nv), ("label_valid", nv)):       # one overwritten poison byte of each compact list
        bad = {n: a.copy() for n, a in good.items()}
        bad[k][at] = 0
        with pytest.raises(AssertionError, match="beyond n_valid"):
            G.check_narrow(cs, bad, refs, cap, "poison of " + k)
    bad = {n: a.copy() for n, a in good.items()}
    bad["inst_idx"][0, need] = 0
    with pytest.raises(AssertionError, match="beyond the lists"):
        G.check_narrow(cs, bad, refs, cap, "poison of inst_idx")


def test_checker_reports_first_match_wide_maps_and_label_errors(seqs, exps):
    seen = set()
    for q in seqs:
        for op, e in zip(q.ops, exps[q.seed, "off"]):
            k = op["kind"]
            if k == "first_match" and k not in seen and int(e["ref"]["off"][-1]) and any(len(r["car_idx"]) and len(r["bg_idx"]) for r in e["ref"]["per"]):
                good = G.forge_first_match(e["ref"], e["frames"], op["colors"])
                G.check_first_match(good, e["ref"], e["frames"], op["colors"], "forged", True)
                f = next(f for f, r in enumerate(e["ref"]["per"]) if len(r["car_idx"]) and len(r["bg_idx"]))
                a = int(e["ref"]["off"][f])
                for name in G.FM_SHAPES:
                    bad = {n: v.copy() for n, v in good.items()}
                    bad[name].reshape(-1).view(np.uint8)[a * bad[name][0:1].nbytes] ^= 1
                    with pytest.raises(AssertionError):
                        G.check_first_match(bad, e["ref"], e["frames"], op["colors"], "wrong " + name, True)
                for name, part in G.FM_PER_POINT.items():
                    n = len(e["ref"]["per"][f][part + "_idx"])
                    bad = {n_: v.copy() for n_, v in good.items()}
                    bad[name][a + n] = 0
                    with pytest.raises(AssertionError, match="beyond the frame's count"):
                        G.check_first_match(bad, e["ref"], e["frames"], op["colors"], "poison of " + name, True)
                bad = {n: v.copy() for n, v in good.items()}
                bad["mask_count"][f, 0] += 1
                with pytest.raises(AssertionError):
                    G.check_first_match(bad, e["ref"], e["frames"], op["colors"], "wrong mask_count", True)
                seen.add(k)
            if k == "wide" and k not in seen and any(r["n_labelled"] for r in e["refs"]):
                G.check_wide(op, e["refs"], e["refs"], "same")
                f = next(f for f, r in enumerate(e["refs"]) if r["n_labelled"])
                bad = [dict(r) for r in e["refs"]]
                bad[f]["label_words"] = bad[f]["label_words"].copy()
                bad[f]["label_words"][np.flatnonzero(bad[f]["label_words"].any(axis=1))[0]] ^= 1
                with pytest.raises(AssertionError):
                    G.check_wide(op, bad, e["refs"], "one wrong label word")
                seen.add(k)
            if k == "depth_maps" and k not in seen and any(len(c[0]) for fr in e["maps"] for c in fr):
                G.check_maps(e["maps"], e["maps"], "same")
                bad = [[tuple(np.array(x) for x in c) for c in fr] for fr in e["maps"]]
                f, m = next((f, m) for f, fr in enumerate(bad) for m, c in enumerate(fr) if len(c[0]))
                bad[f][m][1][0] = np.nextafter(bad[f][m][1][0], 1e9)
                with pytest.raises(AssertionError):
                    G.check_maps(bad, e["maps"], "one depth off by an ulp")
                seen.add(k)
            if k == "pairs" and k not in seen:
                bad = {n: np.array(v) for n, v in e["ref"].items()}
                G.check_bits(bad, e["ref"], "same")
                name = next(n for n, v in bad.items() if v.size)
                bad[name].reshape(-1).view(np.uint8)[0] ^= 1
                with pytest.raises(AssertionError):
                    G.check_bits(bad, e["ref"], "one wrong byte")
                seen.add(k)
    assert seen == {"first_match", "wide", "depth_maps", "pairs"}


def test_checker_reports_inside_box_points_and_operator_errors(seqs, exps):
    seen = set()
    for q in seqs:
        for op, e in zip(q.ops, exps[q.seed, "off"]):
            k = op["kind"]
            if k == "inside_masks" and k not in seen and e["refuse"] is None:
                f = next((f for f, r in enumerate(e["ref"]["inside"]) if 0 < len(r) < e["cap"] and e["ref"]["matched"][f].any()), None)
                if f is None:
                    continue
                good = G.forge_inside(e)
                G.check_inside(good, e, "forged", True)
                for name in ("inside", "part_idx", "part_xyz"):
                    bad = {n: v.copy() for n, v in good.items()}
                    bad[name][f].reshape(-1).view(np.uint8)[0] ^= 1
                    with pytest.raises(AssertionError):
                        G.check_inside(bad, e, "wrong " + name, True)
                    bad = {n: v.copy() for n, v in good.items()}
                    bad[name][f, len(e["ref"]["inside"][f])] = 0
                    with pytest.raises(AssertionError, match="beyond the frame's lists"):
                        G.check_inside(bad, e, "poison of " + name, True)
                for name in ("n_inside", "matched"):
                    bad = {n: v.copy() for n, v in good.items()}
                    bad[name][f, int(np.argmax(e["ref"]["matched"][f]))] += 1
                    with pytest.raises(AssertionError):
                        G.check_inside(bad, e, "wrong " + name, True)
                seen.add(k)
            if k == "box_points" and k not in seen and e["refuse"] is None:
                f = next((f for f, w in enumerate(e["ref"]["first_box"]) if 0 < len(w) < e["off"][f + 1] - e["off"][f]), None)
                if f is None or not len(e["ref"]["box_points"]):
                    continue
                good = G.forge_box_points(e)
                G.check_box_points(good, e, "forged", True)
                a = int(e["off"][f])
                for name, at in (("box_points", 0), ("box_labelled", 0), ("first_box", a), ("frame_counts", f)):
                    bad = {n: v.copy() for n, v in good.items()}
                    bad[name][at] += 1
                    with pytest.raises(AssertionError):
                        G.check_box_points(bad, e, "wrong " + name, True)
                bad = {n: v.copy() for n, v in good.items()}
                bad["first_box"][a + len(e["ref"]["first_box"][f])] = -1
                with pytest.raises(AssertionError, match="beyond n_valid"):
                    G.check_box_points(bad, e, "poison of first_box", True)
                seen.add(k)
            if k == "operators" and k not in seen:
                G.check_operators(e["ref"], e["ref"], "same")
                for name, want in e["ref"].items():
                    if want.size:
                        bad = {n: np.array(v) for n, v in e["ref"].items()}
                        bad[name].reshape(-1).view(np.uint8)[0] ^= 1
                        with pytest.raises(AssertionError):
                            G.check_operators(bad, e["ref"], "wrong " + name)
                seen.add(k)
    assert seen == {"inside_masks", "box_points", "operators"}


def test_refused_calls_and_lab_settings(seqs, exps):
    """The documented refusals the default seeds meet, under every mode: clear_boxes is followed by a refused inside_masks AND a refused
    box_points (its op makes both calls) and by a rerun that counts no box; make_frame_step_wide is refused behind a batch of several
    frames and runs behind a frame step; depth_overlays runs where every depth is > 0.  The lab settings change the geometry only where
    nothing is owed."""
    for m in G.MODES:
        cleared = wide_ref = wide_run = overlays = 0
        for q in seqs:
            for i, (op, e) in enumerate(zip(q.ops, exps[q.seed, m])):
                if op["kind"] == "clear_boxes":
                    assert e["refuse"] == G.NO_BOXES
                    nxt = exps[q.seed, m][i + 1]
                    assert nxt["kind"] == "rerun" and "boxes" not in nxt["setup"] and all(r["count_mb"].shape[1] == 0 for r in nxt["refs"])
                    cleared += 1
                if op["kind"] == "frame_wide":
                    wide_ref += e["refuse"] == G.OTHER_FRAMES
                    wide_run += e["refuse"] is None and e["ref"]["n_labelled"] > 0
                if op["kind"] == "depth_overlays":
                    overlays += e["refuse"] is None and bool(e["ref"]["max_depth"].any())
        assert cleared >= 4 and wide_ref >= 1 and wide_run >= 2 and overlays >= 2, (m, cleared, wide_ref, wide_run, overlays)
    idle = owed = 0
    for q in seqs:
        for m in G.MODES:
            for i, e in enumerate(exps[q.seed, m]):
                form, budget, most = G.lab_settings(q.seed, i, e["idle"])
                assert (form is None) == (not e["idle"]) and budget >= 0 and most >= 0
                idle += e["idle"]
                owed += not e["idle"]
    assert idle and owed
    forms = {G.lab_settings(q.seed, i, True)[0] for q in seqs for i in range(len(q.ops))}
    assert forms == set(G.LAB_FORMS)


def test_depth_maps_ops_leave_counters_for_the_next_call_to_trip_over(seqs, exps):
    """every depth_maps op runs behind a call with every mask full: some (frame, mask, 1024-pixel tile) counts in that call and has
    no member in the op's own, so a counter that is not zeroed between the two calls changes the op's lists"""
    ops = reach = 0
    for q in seqs:
        for op, e in zip(q.ops, exps[q.seed, "off"]):
            if op["kind"] != "depth_maps":
                continue
            ops += 1
            reach += any(set(np.asarray(p[0]) // 1024) - set(np.asarray(w[0]) // 1024)
                         for fp, fw in zip(e["primer"], e["maps"]) for p, w in zip(fp, fw))
    assert ops >= 3 and reach >= 2, (ops, reach)


def test_checker_reports_device_maps_frame_wide_cams_label_views_and_overlay_errors(seqs, exps):
    seen = set()
    for q in seqs:
        for op, e in zip(q.ops, exps[q.seed, "off"]):
            k = op["kind"]
            if k == "depth_maps" and k not in seen:
                needs = [sum(len(c[0]) for c in fr) for fr in e["maps"]]
                cap = max(needs) + 3
                f = next((f for f, n in enumerate(needs) if n), None)
                if f is None:
                    continue
                good = G.forge_maps_device(e["maps"], cap)
                G.check_maps_device(good, e["maps"], cap, "forged")
                for name in good:                             # one wrong entry, then one overwritten poison byte, of each output
                    bad = {n: v.copy() for n, v in good.items()}
                    bad[name][f:f + 1].reshape(-1).view(np.uint8)[0] ^= 1
                    with pytest.raises(AssertionError):
                        G.check_maps_device(bad, e["maps"], cap, "wrong " + name)
                for name in ("pix", "depth", "point_idx"):
                    bad = {n: v.copy() for n, v in good.items()}
                    bad[name][f, needs[f]] = 0
                    with pytest.raises(AssertionError, match="beyond need"):
                        G.check_maps_device(bad, e["maps"], cap, "poison of " + name)
                bad = {n: v.copy() for n, v in good.items()}
                bad["pix"][len(needs), 0] = 0
                with pytest.raises(AssertionError, match="guard row"):
                    G.check_maps_device(bad, e["maps"], cap, "the guard row")
                tight = G.tight_cap(needs)
                if tight is not None:                         # a frame that overflows: flagged, its lists not compared
                    over = G.forge_maps_device(e["maps"], tight)
                    G.check_maps_device(over, e["maps"], tight, "forged, tight")
                    if needs[-1] > tight:                     # ... and what it would write beyond cap is seen in the guard row
                        over["depth"][len(needs), 0] = 1.0
                        with pytest.raises(AssertionError, match="at or beyond cap"):
                            G.check_maps_device(over, e["maps"], tight, "the last frame overflows into the guard row")
                seen.add(k)
            if k == "frame_wide" and k not in seen and e["refuse"] is None and 0 < e["ref"]["n_valid"] < len(e["pts"]) and e["ref"]["n_labelled"]:
                M, B, n = op["cam"]["M"], e["B"], len(e["pts"])
                good = G.forge_frame_wide(e["ref"], n, M, B, e["cap"])
                G.check_frame_wide(good, e["ref"], M, B, "forged")
                for name, v in good.items():
                    if name == "inst_overflow" or not v.size:
                        continue
                    bad = {n_: a.copy() for n_, a in good.items()}
                    bad[name].reshape(-1).view(np.uint8)[0] ^= 1
                    with pytest.raises(AssertionError):
                        G.check_frame_wide(bad, e["ref"], M, B, "wrong " + name)
                for name in G.FRAME_WIDE_LISTS:
                    bad = {n_: a.copy() for n_, a in good.items()}
                    bad[name][e["ref"]["n_valid"]] = 0
                    with pytest.raises(AssertionError, match="beyond n_valid"):
                        G.check_frame_wide(bad, e["ref"], M, B, "poison of " + name)
                bad = {n_: a.copy() for n_, a in good.items()}
                bad["inst_idx"][-1] = 0
                with pytest.raises(AssertionError, match="beyond the lists"):
                    G.check_frame_wide(bad, e["ref"], M, B, "poison of inst_idx")
                seen.add(k)
            if k == "cams" and ("cams", op["wide"]) not in seen and any(r["n_labelled"] for refs in e["refs"] for r in refs):
                G.check_cams(op, e["refs"], e["refs"], "same") if op["wide"] else None
                cam, f = next((c, f) for c, refs in enumerate(e["refs"]) for f, r in enumerate(refs) if r["n_labelled"])
                word = e["refs"][cam][f]["label_words"][:, 0]
                got = [[dict(r, label_bits=r["label_words"][:, 0] if r["label_words"].shape[1] else np.zeros(len(r["u"]), np.uint32),
                             label_valid=(r["label_words"][:, 0] if r["label_words"].shape[1] else np.zeros(len(r["u"]), np.uint32))[r["valid_idx"]])
                        for r in refs] for refs in e["refs"]]
                G.check_cams(op, got, e["refs"], "same")
                bad = [[dict(r) for r in refs] for refs in got]
                key = "label_words" if op["wide"] else "label_bits"
                bad[cam][f][key] = bad[cam][f][key].copy()
                bad[cam][f][key][np.flatnonzero(word)[0]] ^= 1
                with pytest.raises(AssertionError):
                    G.check_cams(op, bad, e["refs"], "one wrong label of camera %d" % cam)
                with pytest.raises(AssertionError):
                    G.check_cams(op, got[:-1] if len(got) > 1 else [got[0][:-1]], e["refs"], "a camera or a frame missing")
                seen.add(("cams", op["wide"]))
            if k == "label" and k not in seen and e["label"].any():
                G.check_label(e["label"].copy(), e["label"], "same")
                bad = e["label"].copy()
                bad.reshape(-1)[np.flatnonzero(bad.reshape(-1))[0]] ^= 1
                with pytest.raises(AssertionError):
                    G.check_label(bad, e["label"], "one wrong pixel")
                seen.add(k)
            if k in ("box_views", "depth_overlays") and k not in seen and e["refuse"] is None:
                G.check_bits({n: np.array(v) for n, v in e["ref"].items()}, e["ref"], "same")
                for name, want in e["ref"].items():
                    if want.size:
                        bad = {n: np.array(v) for n, v in e["ref"].items()}
                        bad[name].reshape(-1).view(np.uint8)[-1] ^= 1
                        with pytest.raises(AssertionError):
                            G.check_bits(bad, e["ref"], "wrong " + name)
                seen.add(k)
    assert seen == {"depth_maps", "frame_wide", ("cams", False), ("cams", True), "label", "box_views", "depth_overlays"}, seen
