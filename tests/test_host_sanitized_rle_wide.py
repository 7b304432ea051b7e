"""Run-length masks in the wide and multi-camera passes (lpf_wide_input.f32 = LPF_MASKS_RLE), host side under AddressSanitizer +
UndefinedBehaviorSanitizer: lpf_api.hip compiled --offload-host-only and linked against tests/host_san/fake_hip.cpp (the stand-in HIP
runtime) by tests/host_san/Makefile (`make asan DRIVER=drive_rle_wide`; the sanitized lpf_api object is shared by every driver of the
session), driven by tests/host_san/drive_rle_wide.cpp -- a stand-alone program: every refusal of lpf_run_wide, lpf_run_cams and
lpf_run_cams_wide with its message and nothing queued (F, M or erode_iters that do not match the call, on_device 1, f32 3, a run one
pixel past camera 1's image that fits camera 0's), the form refused by lpf_depth_maps and lpf_first_match before `masks` is read, M = 0
and masks without runs with no decode launch, M = 256 with F = 3, two run-length cameras in one pass, growing then shrinking calls, a
pipelined context with a narrow run owed -- the caller's arrays and struct freed right after each call.  The driver runs run-length
masks only, so the fake runtime's trace tells what the form costs: the wide decode ran, no dense pack ran, no dense mask was copied."""
import host_san_run as san


@san.needs_hipcc
def test_wide_rle_host_side_under_asan_and_ubsan(tmp_path_factory, tmp_path):
    exe = san.build(tmp_path_factory, "drive_rle_wide")
    text, every = san.drive(exe, trace=tmp_path / "launches.txt", checks=174)
    lines = [l for l in every if l[0] not in ("copy", "memset")]
    names = [l[0] for l in lines]
    wide = [l for l in lines if "lpf_rle_decode_wide" in l[0]]
    narrow = [l for l in lines if "lpf_rle_decode" in l[0] and "lpf_rle_decode_wide" not in l[0]]
    # the wide decode ran, by blocks of 256 threads; lpf_run_cams decoded with the narrow kernel at one- and four-byte label elements
    assert wide and all(d[4:] == ["256", "1", "1"] for d in wide + narrow)
    for lt in ("IhE", "IjE"):
        assert any(lt in d[0] for d in narrow), lt
    # the full-image run at 1408 x 376: 517 units of 1024 pixels, four per block
    assert any(d[1] == str((-(-1408 * 376 // 1024) + 3) // 4) for d in wide)
    # no dense pack of any path ran: the driver gives run-length masks only
    for dense in ("lpf_wide_pack", "lpf_pack16", "lpf_pack_erode", "lpf_wide_direct_project"):
        assert not any(dense in n for n in names), dense
    # erosion is the packed image's, one launch per iteration: the cross and the k x k element, at 32-bit planes behind the wide decode
    eroders = {n for n in names if "erode" in n}
    assert eroders and all("lpf_erode_packed" in n for n in eroders), eroders
    assert any("lpf_erode_packed_k" in n for n in eroders)
    i = next(k for k, n in enumerate(names) if "lpf_rle_decode_wide" in n and k + 2 < len(names) and "lpf_erode_packed" in names[k + 1])
    assert "lpf_erode_packed" in names[i + 1] and "IjE" in names[i + 1] and "lpf_erode_packed" in names[i + 2]
    # no copy of the dense masks' size was made for any successful call (the driver prints what each one's dense twin would have
    # copied), and the largest host-to-device copy of the whole run -- a table of the M = 256, F = 3 call -- is far below that call's
    # 653 568 bytes of dense masks
    would = {int(m) for m in (line.split()[1] for line in text.splitlines() if line.startswith("dense-bytes "))}
    assert len(would) >= 10 and 3 * 256 * 37 * 23 in would
    h2d = [int(l[2]) for l in every if l[0] == "copy" and l[1] == "1"]
    # (twins of a few KB are left out: a table of a few hundred bytes can have the size of five masks of 600 pixels by chance)
    assert h2d and not {w for w in would if w >= 30000} & set(h2d), sorted({w for w in would if w >= 30000} & set(h2d))
    assert max(h2d) < 3 * 256 * 37 * 23 // 2
    # the planes are zeroed in full before a decode: F * LW * H * W * 4 bytes (M = 256, F = 3: eight words per pixel)
    assert any(l[0] == "memset" and int(l[1]) == 3 * 8 * 37 * 23 * 4 for l in every)
