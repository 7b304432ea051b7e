// drive_erosion.cpp -- drives lpf_set_erosion_element's HOST side (lpf_api.hip compiled --offload-host-only against fake_hip.cpp)
// under AddressSanitizer + UndefinedBehaviorSanitizer: the refused sizes and their messages, a NULL context, the default, and
// set -> lpf_set_masks_* -> run with k = 5, k = 3 and k = 1 through the narrow path, lpf_run_wide, lpf_depth_maps and
// lpf_erode_masks_u8.  Kernel launches do nothing here (fake_hip.cpp): they are counted, and their names go to the FAKE_HIP_TRACE
// file, by which tests/test_host_sanitized_erosion.py checks which kernels each element launches; the values are checked on the GPU
// by tests/test_gpu_erosion_element.py.
#include "drive_common.h"

static void refusals(lpf_ctx *c)
{
    CHECK(lpf_set_erosion_element(nullptr, 3) == LPF_ERR_ARG);
    CHECK(lpf_set_erosion_element(nullptr, 4) == LPF_ERR_ARG);
    const int bad[] = {0, 2, 4, 6, 14, 16, 17, -1, -3, 255, 1 << 30};
    for (int k : bad) {
        char want[160];
        snprintf(want, sizeof want, "lpf_set_erosion_element: ksize=%d (the k x k MORPH_ELLIPSE for odd k, 1 .. 15)", k);
        CHECK(lpf_set_erosion_element(c, k) == LPF_ERR_ARG && err_is(want));
    }
    for (int k = 1; k <= 15; k += 2) CHECK(lpf_set_erosion_element(c, k) == LPF_OK);
    CHECK(lpf_set_erosion_element(c, 3) == LPF_OK);
    // host state only: nothing was launched, with or without a camera
    CHECK(fake_hip_launches() == 0);
}

// launches of lpf_set_masks_u8 with `iters` iterations on a W x H image, host masks
static long long pack_launches(lpf_ctx *c, int W, int H, int iters, bool f32 = false)
{
    const int F = 2, M = 9;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    std::vector<uint8_t> masks((size_t)F * M * W * H, 1);
    std::vector<float> fmasks(f32 ? masks.size() : 0, 1.0f);
    const long long l0 = fake_hip_launches();
    if (f32) CHECK(lpf_set_masks_f32(c, fmasks.data(), F, M, 1, iters, 0) == LPF_OK);
    else CHECK(lpf_set_masks_u8(c, masks.data(), F, M, iters, 0) == LPF_OK);
    const long long launches = fake_hip_launches() - l0;
    std::vector<uint32_t> img((size_t)F * W * H);
    CHECK(lpf_get_label_image(c, img.data(), 0) == LPF_OK);
    return launches;
}

static void narrow(lpf_ctx *c)
{
    // the default is the cross: the streaming pack + one launch per iteration where hw % 16 == 0, else the tiled pack with the first
    // iteration fused
    CHECK(pack_launches(c, 128, 48, 2) == 3);
    CHECK(pack_launches(c, 33, 17, 2) == 2);
    CHECK(lpf_set_erosion_element(c, 5) == LPF_OK);          // k x k: always the tiled pack with the first iteration fused
    CHECK(pack_launches(c, 128, 48, 2) == 2);
    CHECK(pack_launches(c, 33, 17, 3) == 3);
    CHECK(pack_launches(c, 33, 17, 1, true) == 1);
    CHECK(lpf_set_erosion_element(c, 15) == LPF_OK);
    CHECK(pack_launches(c, 1, 1, 2) == 2);
    CHECK(lpf_set_erosion_element(c, 16) == LPF_ERR_ARG);    // refused: the element stays 15 x 15
    CHECK(pack_launches(c, 128, 48, 1) == 1);
    CHECK(lpf_set_erosion_element(c, 1) == LPF_OK);          // the identity: packed as without erosion
    CHECK(pack_launches(c, 128, 48, 4) == 1);
    CHECK(pack_launches(c, 33, 17, 4) == 1);
    CHECK(lpf_set_erosion_element(c, 3) == LPF_OK);          // and back
    CHECK(pack_launches(c, 128, 48, 2) == 3);
    CHECK(pack_launches(c, 33, 17, 2) == 2);

    // set -> set_masks -> run, k = 5 then k = 3
    const int W = 128, H = 48, F = 3, M = 5;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    Dev D;
    const int64_t off[F + 1] = {0, 1000, 1000, 4321};
    std::vector<float> pts(4 * off[F], 1.0f);
    std::vector<uint8_t> masks((size_t)F * M * W * H, 1);
    std::vector<double> corners(24 * 7, 0.5);
    const int32_t boff[F + 1] = {0, 3, 3, 7};
    lpf_outputs o;
    memset(&o, 0, sizeof o);
    o.uv = D.get<int32_t>(2 * off[F]); o.label_bits = D.get<uint32_t>(off[F]); o.valid_idx = D.get<int64_t>(off[F]);
    o.inst_idx = D.get<int64_t>((size_t)F * 5000); o.inst_cap = 5000; o.count_mb = D.get<int32_t>((size_t)M * 7);
    o.summary = D.get<lpf_frame_summary>(F);
    CHECK(lpf_set_boxes(c, corners.data(), boff, F, 1) == LPF_OK);
    for (int k : {5, 3}) {
        CHECK(lpf_set_erosion_element(c, k) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, masks.data(), F, M, 2, 0) == LPF_OK);
        CHECK(lpf_run_batch(c, pts.data(), off, F, 0, &o) == LPF_OK);
        uint8_t *dmasks = D.get<uint8_t>(masks.size());      // lent device masks, pipelined
        CHECK(lpf_set_pipelined(c, 2) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, dmasks, F, M, 1, 2) == LPF_OK);
        CHECK(lpf_run_batch(c, pts.data(), off, F, 0, &o) == LPF_OK);
        CHECK(lpf_set_pipelined(c, 0) == LPF_OK);
    }
}

static void wide_and_values(lpf_ctx *c)
{
    const int W = 70, H = 20, F = 2, M = 40;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    Dev D;
    const int64_t off[F + 1] = {0, 1500, 2500}, n = off[F];
    std::vector<float> pts(4 * n, 1.0f);
    std::vector<float> fmasks((size_t)F * M * W * H, 1.0f);
    lpf_wide_input in;
    memset(&in, 0, sizeof in);
    in.masks = fmasks.data(); in.M = M; in.f32 = 1; in.binarize = 1; in.on_device = 0;
    lpf_wide_outputs ow;
    memset(&ow, 0, sizeof ow);
    ow.uv = D.get<int32_t>(2 * n); ow.label_words = D.get<uint32_t>(n * 2); ow.n_valid = D.get<int64_t>(F); ow.n_labelled = D.get<int64_t>(F);
    lpf_depth_maps_outputs dm;
    memset(&dm, 0, sizeof dm);
    dm.cap = 500; dm.pix = D.get<int64_t>((size_t)F * 500); dm.depth = D.get<double>((size_t)F * 500);
    dm.point_idx = D.get<int64_t>((size_t)F * 500); dm.car_off = D.get<int64_t>((size_t)F * (M + 1));
    dm.need = D.get<int64_t>(F); dm.overflow = D.get<int32_t>(F);
    std::vector<uint8_t> small((size_t)2 * 20 * 50, 255), er(small.size());
    for (int k : {5, 3, 1, 15}) {
        CHECK(lpf_set_erosion_element(c, k) == LPF_OK);
        for (int iters = 0; iters < 3; ++iters) {
            in.erode_iters = iters;
            CHECK(lpf_run_wide(c, pts.data(), off, F, 0, &in, &ow) == LPF_OK);
            CHECK(lpf_depth_maps(c, pts.data(), off, F, 0, &in, &dm) == LPF_OK);
            const long long l0 = fake_hip_launches();
            CHECK(lpf_erode_masks_u8(c, small.data(), 2, 20, 50, iters, er.data(), 0) == LPF_OK);
            CHECK(fake_hip_launches() - l0 == (k == 1 ? 0 : iters));
            if (k == 1 || iters == 0) CHECK(memcmp(er.data(), small.data(), small.size()) == 0);      // (the identity is a copy)
        }
    }
    CHECK(lpf_set_erosion_element(c, 3) == LPF_OK);
}

int main()
{
    lpf_ctx *c = drive_begin();
    refusals(c);
    narrow(c);
    wide_and_values(c);
    lpf_destroy(c);
    return drive_finish("drive_erosion", false);
}
