"""Instance-ID maps (lpf_set_masks_ids, lpf_run_wide_ids), host side under AddressSanitizer + UndefinedBehaviorSanitizer: lpf_api.hip
compiled --offload-host-only and linked against tests/host_san/fake_hip.cpp (the stand-in HIP runtime) by tests/host_san/Makefile
(`make asan DRIVER=drive_ids`; the sanitized lpf_api object is shared by every driver of the session), driven by
tests/host_san/drive_ids.cpp -- a stand-alone program: every refusal of both calls with its message and nothing queued, the state
errors, F = 0 and M = 0 with no decode launch, growing then shrinking calls, both ID types, host and device maps, both pipelined modes
with a narrow run owed -- sel, host ids and the struct scribbled over and freed right after each call.  `drive_ids ids` gives ID maps
only, so the fake runtime's trace tells what the form costs: the new kernels ran with the expected grids, no memset of what they write
precedes them, no pack and no run-length decode ran, no dense mask was copied, erosion is the packed image's.  `drive_ids mixed` then
runs lpf_run_wide with dense masks after lpf_run_wide_ids on one context."""
import host_san_run as san


@san.needs_hipcc
def test_id_maps_host_side_under_asan_and_ubsan(tmp_path_factory, tmp_path):
    exe = san.build(tmp_path_factory, "drive_ids")
    text, every = san.drive(exe, "ids", trace=tmp_path / "launches_ids.txt", checks=211)
    lines = [l for l in every if l[0] not in ("copy", "memset")]
    names = [l[0] for l in lines]
    label = [l for l in lines if "lpf_ids_label" in l[0]]
    planes = [l for l in lines if "lpf_ids_planes" in l[0]]
    # all six instantiations of the narrow decode and both of the wide one ran, by one-dimensional grids of blocks of 256 threads
    for it in "ti":
        for lt in "htj":
            assert any("lpf_ids_labelI%s%sE" % (it, lt) in d[0] for d in label), (it, lt)
        assert any("lpf_ids_planesI%sE" % it in d[0] for d in planes), it
    assert all(d[2:] == ["1", "1", "256", "1", "1"] for d in label + planes)
    # 37 x 23: one block per frame (F = 1, 2, 3, 8); 1408 x 376: 259 blocks per uint16 frame, 517 per int32 frame (two frames: 1034)
    assert {d[1] for d in label} == {"1", "2", "3", "8", "259", "1034"} and {d[1] for d in planes} == {"1", "2", "3", "259", "1034"}
    assert any("lpf_ids_labelIthE" in d[0] and d[1] == "259" for d in label) and any("lpf_ids_labelIijE" in d[0] and d[1] == "1034" for d in label)
    assert any("lpf_ids_planesItE" in d[0] and d[1] == "259" for d in planes) and any("lpf_ids_planesIiE" in d[0] and d[1] == "1034" for d in planes)
    # no pack of any path and no run-length decode ran: the driver gives ID maps only
    for other in ("lpf_wide_pack", "lpf_pack16", "lpf_pack_erode", "lpf_wide_direct_project", "lpf_rle_decode"):
        assert not any(other in n for n in names), other
    # erosion is the packed image's, one launch per iteration: the cross and the k x k element, at every element width
    eroders = {n for n in names if "erode" in n}
    assert eroders and all("lpf_erode_packed" in n for n in eroders), eroders
    assert any("lpf_erode_packed_k" in n for n in eroders)
    for lt in ("IhE", "ItE", "IjE"):
        assert any(lt in n for n in eroders), lt
    i = next(k for k, n in enumerate(names) if "lpf_ids_label" in n and k + 2 < len(names) and "lpf_erode_packed" in names[k + 1])
    assert "lpf_erode_packed" in names[i + 2] and "lpf_ids" not in names[i + 2]
    # nothing the decodes write is zeroed first: the only memsets are the zeroed images of the M = 0 calls (F = 5: 5 * 851 bytes), and
    # no memset has the size of an image or of the planes that a successful call wrote
    said = [line.split() for line in text.splitlines()]
    written = {int(l[1]) for l in said if l and l[0] == "written-bytes"}
    memsets = [int(l[1]) for l in every if l[0] == "memset"]
    assert len(written) >= 10 and 3 * 8 * 37 * 23 * 4 in written and 5 * 37 * 23 in memsets
    assert not written & set(memsets), sorted(written & set(memsets))
    for k, l in enumerate(every):
        if "lpf_ids_" in l[0]:
            assert every[k - 1][0] != "memset", every[k - 1]
    # no copy of the dense masks' size was made for any successful call (the driver prints what each one's dense twin would have
    # copied); the largest host-to-device copy of the whole run is a map: 2 frames of 1408 x 376 int32
    would = {int(l[1]) for l in said if l and l[0] == "dense-bytes"}
    h2d = [int(l[2]) for l in every if l[0] == "copy" and l[1] == "1"]
    assert len(would) >= 10 and 3 * 256 * 37 * 23 in would
    assert h2d and not {w for w in would if w >= 30000} & set(h2d), sorted({w for w in would if w >= 30000} & set(h2d))
    assert max(h2d) == 2 * 1408 * 376 * 4
    # dense masks after ID maps on the same context, and ID maps after them: the dense pack runs again, beside the new decodes
    text, every = san.drive(exe, "mixed", trace=tmp_path / "launches_mixed.txt", checks=9)
    names = [l[0] for l in every]
    assert any("lpf_wide_pack" in n for n in names) and sum("lpf_ids_planes" in n for n in names) == 2
    assert sum("lpf_ids_label" in n for n in names) == 2
