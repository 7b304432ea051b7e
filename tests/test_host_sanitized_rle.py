"""lpf_set_masks_rle's host side under AddressSanitizer + UndefinedBehaviorSanitizer: lpf_api.hip compiled --offload-host-only and linked
against tests/host_san/fake_hip.cpp (the stand-in HIP runtime) by tests/host_san/Makefile (`make asan DRIVER=drive_rle`: the sanitized
lpf_api object is built once per session and shared by every driver), driven by tests/host_san/drive_rle.cpp -- a stand-alone program:
every refusal with its message (start = length = INT32_MAX, run_off[0] = 1 and a run_off that decreases among them) and nothing queued
by any, the state errors (no camera, inside a capture), F = 0 / M = 0 / no runs without a decode launch, erode_iters = 2 as decode + 2
erosions, 10^5 runs, growing then shrinking calls, the pipelined modes, and the caller's arrays freed right after each call.  The fake
runtime's launch trace tells which kernels ran."""
import host_san_run as san


@san.needs_hipcc
def test_set_masks_rle_host_side_under_asan_and_ubsan(tmp_path_factory, tmp_path):
    exe = san.build(tmp_path_factory, "drive_rle")
    text, every = san.drive(exe, trace=tmp_path / "launches.txt", checks=98)
    lines = [l for l in every if l[0] not in ("copy", "memset")]
    names = [l[0] for l in lines]
    decodes = [l for l in lines if "lpf_rle_decode" in l[0]]
    # the three label element widths were decoded, by blocks of 256 threads
    for lt in ("IhE", "ItE", "IjE"):
        assert any(lt in d[0] for d in decodes), lt
    assert all(d[4:] == ["256", "1", "1"] for d in decodes)
    # the full-image run at 1408 x 376: 517 units of 1024 pixels, four per block
    assert any(d[1] == str((-(-1408 * 376 // 1024) + 3) // 4) for d in decodes)
    # erosion after a decode is the packed image's: the cross and the k x k element, never a pack with a fused first iteration
    i = next(k for k, n in enumerate(names) if "lpf_rle_decode" in n and k + 2 < len(names) and "lpf_erode_packed" in names[k + 1])
    assert "lpf_erode_packed" in names[i + 1] and "lpf_erode_packed" in names[i + 2]
    assert any("lpf_erode_packed_k" in n for n in names)
    assert not any("lpf_pack_erode_k" in n for n in names)
