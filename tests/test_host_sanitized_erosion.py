"""lpf_set_erosion_element's host side under AddressSanitizer + UndefinedBehaviorSanitizer: lpf_api.hip compiled --offload-host-only and
linked against tests/host_san/fake_hip.cpp (the stand-in HIP runtime) by tests/host_san/Makefile (`make asan DRIVER=drive_erosion`: the
sanitized lpf_api object is built once per session and shared by every driver), driven by tests/host_san/drive_erosion.cpp: the
refused sizes and their messages, a NULL context, the default, and set -> set_masks -> run with k = 5, 3, 1 and 15 through the narrow
path, lpf_run_wide, lpf_depth_maps and lpf_erode_masks_u8.  The fake runtime's launch trace tells which kernels ran: the cross
launches the 3x3 kernels only, another size the k x k ones."""
import host_san_run as san


@san.needs_hipcc
def test_erosion_element_host_side_under_asan_and_ubsan(tmp_path_factory, tmp_path):
    exe = san.build(tmp_path_factory, "drive_erosion")
    text, every = san.drive(exe, trace=tmp_path / "launches.txt", checks=149)
    names = [l[0] for l in every if l[0] not in ("copy", "memset")]
    # the driver starts with the default element (two set_masks calls of two iterations, at 128 x 48 and at 33 x 17): the streaming
    # pack and two erosions, the tiled pack with its fused first erosion and one more -- the 3x3 kernels, none of the k x k ones
    first_k = next(i for i, n in enumerate(names) if "lpf_pack_erode_k" in n)
    head = names[:first_k]
    assert [n.split("I")[0].lstrip("_Z0123456789") for n in head] == ["lpf_pack16", "lpf_erode_packed", "lpf_erode_packed", "lpf_pack_erode",
                                                                     "lpf_erode_packed"], head
    for kernel in ("lpf_pack_erode_k", "lpf_erode_packed_k", "lpf_wide_pack_k", "lpf_erode_u8_k_kernel", "lpf_wide_packI", "lpf_erode_u8_kernel"):
        assert any(kernel in n for n in names), kernel
