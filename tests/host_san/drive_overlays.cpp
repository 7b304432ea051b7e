// drive_overlays.cpp -- drives lpf_depth_overlays' HOST side (lpf_api.hip compiled --offload-host-only against fake_hip.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: its refused arguments and their messages, host and device lists, segmented images
// and outputs, and the chunk loop (a 1408 x 376 frame of 200 cars with host outputs is 318 MB: two chunks of at most 256 MiB).
// Kernel launches do nothing here (fake_hip.cpp): the launches are counted, the images are checked on the GPU by
// tests/test_gpu_depth_overlays.py.
#include "drive_common.h"
#include <cmath>

struct Lists {                    // F frames of M cars: car m of frame f holds `per` ascending pixels, with depths 1 .. per
    int F, M;
    int64_t cap;
    std::vector<int64_t> pix, off;
    std::vector<double> depth;
    Lists(int F_, int M_, int per, int64_t hw) : F(F_), M(M_), cap((int64_t)M_ * per + 3)
    {
        pix.assign((size_t)F * cap, 0); depth.assign((size_t)F * cap, 0.0); off.assign((size_t)F * (M + 1), 0);
        for (int f = 0; f < F; ++f)
            for (int m = 0; m < M; ++m) {
                const int64_t a = (int64_t)m * per;
                off[(size_t)f * (M + 1) + m + 1] = a + per;
                for (int k = 0; k < per; ++k) {
                    pix[(size_t)f * cap + a + k] = (int64_t)k * (hw / (per + 1)) + (m % 3);
                    depth[(size_t)f * cap + a + k] = 1.0 + k;
                }
            }
    }
    lpf_depth_overlay_input input(const uint8_t *seg, int on_device) const
    {
        lpf_depth_overlay_input in;
        memset(&in, 0, sizeof in);
        in.pix = pix.data(); in.depth = depth.data(); in.cap = cap; in.car_off = off.data(); in.M = M;
        in.lists_on_device = on_device; in.seg = seg; in.seg_on_device = on_device;
        return in;
    }
};

static void refusals(lpf_ctx *c)
{
    const int W = 64, H = 48;
    Lists L(2, 3, 5, (int64_t)W * H);
    std::vector<uint8_t> seg((size_t)2 * W * H * 3, 9), img((size_t)2 * 3 * W * H * 3);
    std::vector<double> mx(6);
    lpf_depth_overlay_outputs o;
    memset(&o, 0, sizeof o);
    o.images = img.data(); o.max_depth = mx.data();
    lpf_depth_overlay_input in = L.input(seg.data(), 0);
    CHECK(lpf_depth_overlays(nullptr, 1, &in, &o) == LPF_ERR_ARG);
    CHECK(lpf_depth_overlays(c, 1, &in, &o) == LPF_ERR_STATE && err_starts("lpf_set_camera has not been called"));
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 30) == LPF_OK);
    CHECK(lpf_depth_overlays(c, 2, &in, &o) == LPF_OK);
    CHECK(lpf_depth_overlays(c, -1, &in, &o) == LPF_ERR_ARG && err_starts("depth_overlays: in="));
    CHECK(lpf_depth_overlays(c, 1, nullptr, &o) == LPF_ERR_ARG && lpf_depth_overlays(c, 1, &in, nullptr) == LPF_ERR_ARG);
    lpf_depth_overlay_input b = in;
    b.M = 257;
    CHECK(lpf_depth_overlays(c, 1, &b, &o) == LPF_ERR_ARG &&
          err_starts("depth_overlays: M=257 cars per frame, lpf_depth_overlays takes 0 .. LPF_MAX_MASKS_WIDE = 256"));
    b = in; b.cap = -1;
    CHECK(lpf_depth_overlays(c, 1, &b, &o) == LPF_ERR_ARG && err_starts("depth_overlays: cap=-1"));
    b = in; b.car_off = nullptr;
    CHECK(lpf_depth_overlays(c, 1, &b, &o) == LPF_ERR_ARG);
    b = in; b.seg = nullptr;
    CHECK(lpf_depth_overlays(c, 1, &b, &o) == LPF_ERR_ARG);
    b.M = 0;                                                          // no cars: seg may be NULL
    CHECK(lpf_depth_overlays(c, 1, &b, &o) == LPF_OK);
    b = in; b.pix = nullptr;
    CHECK(lpf_depth_overlays(c, 1, &b, &o) == LPF_ERR_ARG);
    b = in; b.depth = nullptr;
    CHECK(lpf_depth_overlays(c, 1, &b, &o) == LPF_ERR_ARG);
    lpf_depth_overlay_outputs none;
    memset(&none, 0, sizeof none);
    CHECK(lpf_depth_overlays(c, 1, &in, &none) == LPF_ERR_ARG && err_starts("depth_overlays: images and max_depth are both NULL"));
    // host lists that fail their checks
    Lists bad = L;
    bad.off[2] = bad.off[1] - 1;                                      // decreasing at car 1
    lpf_depth_overlay_input bi = bad.input(seg.data(), 0);
    CHECK(lpf_depth_overlays(c, 1, &bi, &o) == LPF_ERR_ARG && err_starts("depth_overlays: frame 0: car_off decreases at car 1"));
    bad = L; bad.off[3] = bad.cap + 1;
    bi = bad.input(seg.data(), 0);
    CHECK(lpf_depth_overlays(c, 1, &bi, &o) == LPF_ERR_ARG && err_starts("depth_overlays: frame 0: car_off 0 .. "));
    bad = L; bad.pix[2] = bad.pix[1];
    bi = bad.input(seg.data(), 0);
    CHECK(lpf_depth_overlays(c, 1, &bi, &o) == LPF_ERR_ARG && err_starts("depth_overlays: frame 0 car 0: pixel"));
    bad = L; bad.pix[(size_t)bad.cap + 5] = (int64_t)W * H;           // frame 1, car 1's first entry: outside the image
    bi = bad.input(seg.data(), 0);
    CHECK(lpf_depth_overlays(c, 2, &bi, &o) == LPF_ERR_ARG && err_starts("depth_overlays: frame 1 car 1: pixel 3072"));
    bad = L; bad.depth[7] = NAN;
    bi = bad.input(seg.data(), 0);
    CHECK(lpf_depth_overlays(c, 1, &bi, &o) == LPF_ERR_ARG && err_starts("depth_overlays: frame 0 car 1: depth nan"));
    bad = L; bad.depth[3] = -2.0;
    bi = bad.input(seg.data(), 0);
    CHECK(lpf_depth_overlays(c, 1, &bi, &o) == LPF_ERR_ARG && err_starts("depth_overlays: frame 0 car 0: depth -2"));
    // device lists are not checked (the kernels clamp them): the same bad lists are taken
    bi = bad.input(seg.data(), 1);
    o.on_device = 1;
    CHECK(lpf_depth_overlays(c, 1, &bi, &o) == LPF_OK);
    o.on_device = 0;
    // F = 0 and M = 0 do nothing
    CHECK(lpf_depth_overlays(c, 0, &in, &o) == LPF_OK);
    // while a graph is captured the call is refused
    CHECK(lpf_graph_begin(c) == LPF_OK);
    CHECK(lpf_depth_overlays(c, 1, &in, &o) == LPF_ERR_STATE && err_starts("lpf_depth_overlays cannot be captured"));
    CHECK(lpf_depth_overlays(c, 2, &in, &o) == LPF_OK);               // (the refusal abandoned the capture)
}

// host and device memory in every combination; only max_depth; and the chunk loop
static void runs(lpf_ctx *c)
{
    {
        const int W = 128, H = 48, F = 3, M = 4;
        Lists L(F, M, 6, (int64_t)W * H);
        std::vector<uint8_t> seg((size_t)F * W * H * 3, 3), img((size_t)F * M * W * H * 3);
        std::vector<double> mx((size_t)F * M);
        CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 30) == LPF_OK);
        for (int lists_dev = 0; lists_dev < 2; ++lists_dev)
            for (int seg_dev = 0; seg_dev < 2; ++seg_dev)
                for (int out_dev = 0; out_dev < 2; ++out_dev)
                    for (int want_img = 0; want_img < 2; ++want_img) {
                        lpf_depth_overlay_input in = L.input(seg.data(), lists_dev);
                        in.seg_on_device = seg_dev;
                        lpf_depth_overlay_outputs o;
                        memset(&o, 0, sizeof o);
                        o.images = want_img ? img.data() : nullptr; o.max_depth = mx.data(); o.on_device = out_dev;
                        const long long l0 = fake_hip_launches();
                        CHECK(lpf_depth_overlays(c, F, &in, &o) == LPF_OK);
                        CHECK(fake_hip_launches() - l0 == (want_img ? 2 : 1));    // one chunk: render + paint, or paint alone
                    }
    }
    {
        const int W = 1408, H = 376, M = 200;                          // 318 MB of host images: two chunks
        Lists L(1, M, 4, (int64_t)W * H);
        std::vector<uint8_t> seg((size_t)W * H * 3, 5), img((size_t)M * W * H * 3);
        std::vector<double> mx(M);
        CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 30) == LPF_OK);
        lpf_depth_overlay_input in = L.input(seg.data(), 0);
        lpf_depth_overlay_outputs o;
        memset(&o, 0, sizeof o);
        o.images = img.data(); o.max_depth = mx.data();
        const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
        CHECK(lpf_depth_overlays(c, 1, &in, &o) == LPF_OK);
        CHECK(fake_hip_launches() - l0 == 4);                          // two chunks of render + paint
        CHECK(fake_hip_copies() - c0 == 2 * 5 + 1);                    // per chunk: seg, pix, depth, car_off up, images down; max_depth
        o.on_device = 1;                                               // device outputs and host inputs: the inputs' staging bounds the chunk
        const long long l1 = fake_hip_launches();
        CHECK(lpf_depth_overlays(c, 1, &in, &o) == LPF_OK);
        CHECK(fake_hip_launches() - l1 == 2);
    }
}

int main()
{
    lpf_ctx *c = drive_begin();
    refusals(c);
    runs(c);
    lpf_destroy(c);
    return drive_finish("drive_overlays", true);
}
