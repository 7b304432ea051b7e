"""lpf_depth_maps_rle and lpf_first_match_rle, host side under AddressSanitizer + UndefinedBehaviorSanitizer: lpf_api.hip compiled
--offload-host-only and linked against tests/host_san/fake_hip.cpp (the stand-in HIP runtime) by tests/host_san/Makefile (`make asan
DRIVER=drive_rle_analysis`; the sanitized lpf_api object is shared by every driver of the session), driven by
tests/host_san/drive_rle_analysis.cpp -- a stand-alone program: every refusal of both calls with its message and nothing queued (a bad run
in the last frame of a batch of several ranges, masks->F != F, erode_iters = 1 for first match, a run one pixel past mh x mw that fits
the camera's image), M = 0 and masks without runs with no decode launch, growing then shrinking calls, a pipelined context with a
narrow run owed -- the caller's arrays and structs freed right after each call.  The driver runs run-length masks only, so the fake
runtime's trace tells what the form costs; its multi-range section (17 frames of 256 masks at 1408 x 376: 16.9 MB of planes per frame
against the 256 MiB of a range) stands between marker lines."""
import host_san_run as san
F, M, HW, LW = 17, 256, 1408 * 376, 8                       # the multi-range batch of the driver (several_ranges)


def _ranges(section):
    """The ranges of one call's trace lines: per decode launch (zeroed plane bytes, bytes of the runs table, decode blocks)."""
    out = []
    for i, l in enumerate(section):
        if "lpf_rle_decode_wide" in l[0]:
            # the range, as wide_pack queues it: memset planes | copy runs | copy units | copy run_off | decode
            assert [x[0] for x in section[i - 4:i]] == ["memset", "copy", "copy", "copy"], section[i - 4:i + 1]
            assert section[i - 3][1] == section[i - 2][1] == section[i - 1][1] == "1"
            out.append((int(section[i - 4][1]), int(section[i - 3][2]), int(section[i - 2][2]), int(section[i - 1][2]), int(l[1])))
    return out


@san.needs_hipcc
def test_rle_analysis_host_side_under_asan_and_ubsan(tmp_path_factory, tmp_path):
    exe = san.build(tmp_path_factory, "drive_rle_analysis")
    text, every = san.drive(exe, trace=tmp_path / "launches.txt", checks=332)
    names = [l[0] for l in every if l[0] not in ("copy", "memset")]
    # the new count kernel and the raster's planes instantiation (uint32, rule 0, PLANES, count and scatter) ran; nothing dense did
    assert any("lpf_fm_count_planes" in n for n in names)
    assert any("lpf_dm_rasterIjLi0ELb1ELb0E" in n for n in names) and any("lpf_dm_rasterIjLi0ELb1ELb1E" in n for n in names)
    assert not any("lpf_fm_countI" in n for n in names)
    assert not any("lpf_dm_raster" in n and "Lb1ELb" not in n for n in names)
    for dense in ("lpf_wide_pack", "lpf_pack16", "lpf_pack_erode"):
        assert not any(dense in n for n in names), dense
    eroders = {n for n in names if "erode" in n}
    assert eroders and all("lpf_erode_packed" in n and "IjE" in n for n in eroders), eroders
    assert any("lpf_erode_packed_k" in n for n in eroders)
    # no copy of the dense masks' size was made for any successful call, and the largest host-to-device copy of the whole run is far
    # below the multi-range batch's 2.3 GB of dense masks -- and below ONE of its frames' 136 MB
    would = {int(m) for m in (line.split()[1] for line in text.splitlines() if line.startswith("dense-bytes "))}
    assert len(would) >= 10 and F * M * HW in would
    h2d = [int(l[2]) for l in every if l[0] == "copy" and l[1] == "1"]
    assert h2d and not {w for w in would if w >= 30000} & set(h2d), sorted({w for w in would if w >= 30000} & set(h2d))
    assert max(h2d) < 1 << 20

    # ---- the multi-range section: first match | depth maps | depth maps with one erosion iteration
    marks = [i for i, l in enumerate(every) if l == ["memset", "7"]]
    assert len(marks) == 4
    sections = [every[a + 1:b] for a, b in zip(marks, marks[1:])]
    for sec, plane_sets in zip(sections, (1, 1, 2)):
        rng = _ranges(sec)
        frames = [blocks * 4 // M for _, _, _, _, blocks in rng]          # one run, one unit per mask: four units per decode block
        assert len(rng) > 1 and sum(frames) == F and all(f > 0 for f in frames), rng
        for (zeroed, b_runs, b_units, b_off, blocks), fc in zip(rng, frames):
            assert blocks * 4 == fc * M                                # the range's decode got its own frames' runs, and only those
            assert b_runs == b_units == fc * M * 8 and b_off == (fc * M + 1) * 8
            assert zeroed == fc * LW * HW * 4                          # the planes are zeroed in full per range
            assert fc * LW * HW * 4 * plane_sets <= 256 << 20            # ... and stay within the staging bound of a range
    fm, dm, dme = sections
    counts = [l for l in fm if "lpf_fm_count_planes" in l[0]]
    assert [int(l[2]) for l in counts] == [b * 4 // M for _, _, _, _, b in _ranges(fm)]       # grid.y: the range's frames
    for sec in (dm, dme):
        rast = [l for l in sec if "lpf_dm_rasterIjLi0ELb1ELb0E" in l[0]]
        assert [int(l[2]) for l in rast] == [b * 4 // M for _, _, _, _, b in _ranges(sec)]
    assert sum(1 for l in dme if "lpf_erode_packedIjE" in l[0]) == len(_ranges(dme)) and not any("erode" in l[0] for l in dm)
