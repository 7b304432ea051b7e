// drive_first_match.cpp -- drives lpf_first_match's HOST side (lpf_api.hip compiled --offload-host-only against fake_hip.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: its refused arguments and their messages, the camera it needs, host and device memory
// for the points, the masks and the outputs in every combination, several selections of outputs, colours or none, F = 0, M = 0, empty
// frames and a batch without points, what goes back to a host caller (the lists as they were where the kernels wrote nothing), a
// repeated all-device call without a host wait, and a batch whose host masks pass the staging bound and go through in two ranges.
// Kernel launches do nothing here (fake_hip.cpp): the launches and copies are counted and the launch lines recorded (FAKE_HIP_TRACE,
// read by tests/test_host_sanitized_first_match.py); the values are checked on the GPU by tests/test_gpu_first_match.py.
#include "drive_common.h"

struct Batch {                    // F frames of the given sizes, M uint8 masks of mh x mw per frame, a colour row per mask
    int F, M, mh, mw;
    std::vector<float> pts;
    std::vector<int64_t> frame_off;
    std::vector<uint8_t> masks;
    std::vector<double> colors;
    Batch(const std::vector<int> &sizes, int M_, int mh_, int mw_) : F((int)sizes.size()), M(M_), mh(mh_), mw(mw_)
    {
        frame_off.push_back(0);
        for (int n : sizes) frame_off.push_back(frame_off.back() + n);
        pts.assign((size_t)frame_off.back() * 4 + 4, 0.5f);
        masks.assign((size_t)F * M * mh * mw + 1, 1);
        colors.assign((size_t)F * M * 3 + 1, 0.25);
    }
    int64_t N() const { return frame_off.back(); }
    lpf_first_match_input input(int on_device, bool with_colors = true) const
    {
        lpf_first_match_input in;
        memset(&in, 0, sizeof in);
        in.masks = M ? masks.data() : nullptr; in.colors = with_colors && M ? colors.data() : nullptr;
        in.M = M; in.mh = mh; in.mw = mw; in.on_device = on_device;
        return in;
    }
};

enum { DENSE = 1, CAR = 2, RGB = 4, BG = 8, NVALID = 16, COUNTS = 32, ALL = 63 };
struct Out {
    std::vector<int32_t> first_mask, car_mask;
    std::vector<int64_t> car_idx, bg_idx, n_valid, n_car, n_bg, mask_count;
    std::vector<float> car_xyz, bg_xyz;
    std::vector<double> car_rgb;
    explicit Out(const Batch &b)
        : first_mask((size_t)b.N() + 1, 7), car_mask((size_t)b.N() + 1, 7), car_idx((size_t)b.N() + 1, 7), bg_idx((size_t)b.N() + 1, 7),
          n_valid((size_t)b.F + 1, 7), n_car((size_t)b.F + 1, 7), n_bg((size_t)b.F + 1, 7), mask_count((size_t)b.F * b.M + 1, 7),
          car_xyz((size_t)b.N() * 3 + 1, 7.f), bg_xyz((size_t)b.N() * 3 + 1, 7.f), car_rgb((size_t)b.N() * 3 + 1, 7.0) {}
    lpf_first_match_outputs outputs(int on_device, unsigned which = ALL)
    {
        lpf_first_match_outputs o;
        memset(&o, 0, sizeof o);
        if (which & DENSE) o.first_mask = first_mask.data();
        if (which & CAR) { o.car_idx = car_idx.data(); o.car_mask = car_mask.data(); o.car_xyz = car_xyz.data(); }
        if (which & RGB) o.car_rgb = car_rgb.data();
        if (which & BG) { o.bg_idx = bg_idx.data(); o.bg_xyz = bg_xyz.data(); }
        if (which & NVALID) o.n_valid = n_valid.data();
        if (which & COUNTS) o.mask_count = mask_count.data();
        o.n_car = n_car.data(); o.n_bg = n_bg.data();
        o.on_device = on_device;
        return o;
    }
    bool lists_untouched() const         // (the fake kernels write nothing: a host caller's lists come back as they went up)
    {
        for (size_t i = 0; i < car_idx.size(); ++i) if (car_idx[i] != 7 || car_mask[i] != 7 || bg_idx[i] != 7) return false;
        for (size_t i = 0; i < car_xyz.size(); ++i) if (car_xyz[i] != 7.f || bg_xyz[i] != 7.f || car_rgb[i] != 7.0) return false;
        return true;
    }
};

static void refusals(lpf_ctx *c)
{
    Batch b({100, 0, 50}, 3, 20, 30);
    Out out(b);
    lpf_first_match_input in = b.input(0);
    lpf_first_match_outputs o = out.outputs(0);
    const float *pts = b.pts.data();
    const int64_t *fo = b.frame_off.data();
    CHECK(lpf_first_match(nullptr, pts, fo, 3, 0, &in, &o) == LPF_ERR_ARG);
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &in, &o) == LPF_ERR_STATE && err_starts("lpf_set_camera has not been called"));
    set_camera(c, 30.0);
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &in, &o) == LPF_OK);
    CHECK(lpf_first_match(c, pts, fo, 0, 0, &in, &o) == LPF_OK);                  // F = 0 does nothing
    CHECK(lpf_first_match(c, pts, fo, -1, 0, &in, &o) == LPF_ERR_ARG && err_starts("first_match: in="));
    CHECK(lpf_first_match(c, pts, fo, 3, 0, nullptr, &o) == LPF_ERR_ARG && err_starts("first_match: in="));
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &in, nullptr) == LPF_ERR_ARG && err_starts("first_match: in="));
    CHECK(lpf_first_match(c, pts, nullptr, 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("first_match: in="));
    CHECK(lpf_first_match(c, nullptr, fo, 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("first_match: pts is NULL"));
    lpf_first_match_input x = in;
    x.M = -1;
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("first_match: M=-1 masks per frame"));
    x.M = LPF_MAX_MASKS_WIDE + 1;
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("first_match: M=257 masks per frame"));
    x = in; x.masks = nullptr;
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("first_match: masks="));
    x = in; x.mh = 0;
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("first_match: masks=") && strstr(lpf_last_error(c), "mh=0"));
    x = in; x.mw = -4;
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && strstr(lpf_last_error(c), "mw=-4"));
    x = in; x.colors = nullptr;
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("first_match: car_rgb is asked for, colors is NULL"));
    lpf_first_match_outputs y = o;
    y.car_rgb = nullptr;
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &x, &y) == LPF_OK);                   // (no colours, no car_rgb: fine)
    y = o; y.n_car = nullptr;
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &in, &y) == LPF_ERR_ARG && err_starts("first_match: n_car="));
    y = o; y.n_bg = nullptr;
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &in, &y) == LPF_ERR_ARG && err_starts("first_match: n_car="));
    std::vector<int64_t> bad = b.frame_off;
    bad[2] = bad[1] - 1;
    CHECK(lpf_first_match(c, pts, bad.data(), 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("first_match: frame 1 has -1 points"));
    bad = b.frame_off; bad[0] = 1;
    CHECK(lpf_first_match(c, pts, bad.data(), 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("first_match: frame_off[0] must be 0"));
    x = in; x.M = 0; x.masks = nullptr; x.mh = x.mw = 0;                          // M = 0: masks, mh and mw are not looked at
    y = o; y.car_rgb = nullptr;
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &x, &y) == LPF_OK);
    // while a graph is captured the call is refused
    CHECK(lpf_graph_begin(c) == LPF_OK);
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &in, &o) == LPF_ERR_STATE && err_starts("lpf_first_match cannot be captured"));
    CHECK(lpf_first_match(c, pts, fo, 3, 0, &in, &o) == LPF_OK);                  // (the refusal abandoned the capture)
}

static int bits(unsigned v) { int n = 0; for (; v; v &= v - 1) ++n; return n; }

// host and device memory in every combination, several selections of outputs; what a host caller gets back
static void runs(lpf_ctx *c)
{
    Batch b({100, 0, 2500, 50}, 3, 20, 30);                                       // frame 1 is empty; frame 2 has three tiles
    const unsigned picks[] = {ALL, ALL & ~RGB, DENSE | NVALID | COUNTS, CAR | BG, BG, 0};
    for (int pts_dev = 0; pts_dev < 2; ++pts_dev)
        for (int in_dev = 0; in_dev < 2; ++in_dev)
            for (int out_dev = 0; out_dev < 2; ++out_dev)
                for (unsigned which : picks) {
                    Out out(b);
                    lpf_first_match_input in = b.input(in_dev, (which & RGB) != 0);
                    lpf_first_match_outputs o = out.outputs(out_dev, which);
                    const bool lists = (which & (CAR | RGB | BG)) != 0;
                    const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
                    CHECK(lpf_first_match(c, b.pts.data(), b.frame_off.data(), b.F, pts_dev, &in, &o) == LPF_OK);
                    CHECK(fake_hip_launches() - l0 == (lists ? 3 : 2));           // count, scan and -- with a list asked for -- scatter
                    // the frame offsets; the points; the masks (and colours); per list array up and back; the dense codes, n_valid, n_car,
                    // n_bg and the mask counts back
                    const int n_lists = ((which & CAR) ? 3 : 0) + ((which & RGB) ? 1 : 0) + ((which & BG) ? 2 : 0);
                    long long copies = 1 + (pts_dev ? 0 : 1) + (in_dev ? 0 : 1 + ((which & RGB) ? 1 : 0));
                    if (!out_dev) copies += 2 * n_lists + bits(which & (DENSE | NVALID | COUNTS)) + 2;
                    CHECK(fake_hip_copies() - c0 == copies);
                    CHECK(out.lists_untouched());
                    CHECK(out.first_mask[(size_t)b.N()] == 7 && out.n_car[(size_t)b.F] == 7 && out.n_bg[(size_t)b.F] == 7 && out.n_valid[(size_t)b.F] == 7);
                    CHECK(out.mask_count[(size_t)b.F * b.M] == 7);
                    if (!out_dev && (which & COUNTS)) CHECK(out.mask_count[0] == 0 && out.mask_count[(size_t)b.F * b.M - 1] == 0);     // (zeroed in stream order)
                }
    {
        // a batch without points, and one without masks: still legal; no count and no scatter launch without points
        Batch np({0, 0}, 2, 8, 8);
        Out out(np);
        lpf_first_match_input in = np.input(0);
        lpf_first_match_outputs o = out.outputs(0);
        const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
        CHECK(lpf_first_match(c, nullptr, np.frame_off.data(), 2, 0, &in, &o) == LPF_OK && fake_hip_launches() == l0 + 1);
        CHECK(fake_hip_copies() - c0 == 1 + 2 + 4);                               // offsets; masks and colours; the three counts and mask_count back
        Batch nm({300, 10}, 0, 0, 0);
        Out out2(nm);
        lpf_first_match_input in2 = nm.input(1);
        lpf_first_match_outputs o2 = out2.outputs(0, ALL & ~RGB);
        CHECK(lpf_first_match(c, nm.pts.data(), nm.frame_off.data(), 2, 0, &in2, &o2) == LPF_OK && fake_hip_launches() == l0 + 4);
        CHECK(out2.lists_untouched());
    }
    {
        // everything on the device: no host wait, no blocking upload, one ring upload (the frame offsets) -- and the second call of
        // the shape allocates nothing (an allocation of a buffer in use would drain first: a host wait)
        Out out(b);
        lpf_first_match_input in = b.input(1);
        lpf_first_match_outputs o = out.outputs(1);
        CHECK(lpf_first_match(c, b.pts.data(), b.frame_off.data(), b.F, 1, &in, &o) == LPF_OK);
        int64_t st[8];
        CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK);
        const long long c0 = fake_hip_copies();
        CHECK(lpf_first_match(c, b.pts.data(), b.frame_off.data(), b.F, 1, &in, &o) == LPF_OK);
        CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK && st[0] == 0 && st[1] == 0 && st[6] == 0 && st[2] == 1);
        CHECK(fake_hip_copies() - c0 == 1);
    }
}

// ten frames of 32 host masks of 1 MiB each: 32 MiB of staging per frame, so a range holds seven frames under the 256 MiB bound and
// the batch goes through as 7 + 3 frames (the launch lines show the two grids)
static void chunks(lpf_ctx *c)
{
    Batch b({10, 2000, 10, 10, 10, 10, 10, 10, 1500, 10}, 32, 1024, 1024);
    Out out(b);
    lpf_first_match_input in = b.input(0, false);
    lpf_first_match_outputs o = out.outputs(0, ALL & ~RGB);
    const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
    CHECK(lpf_first_match(c, b.pts.data(), b.frame_off.data(), b.F, 0, &in, &o) == LPF_OK);
    CHECK(fake_hip_launches() - l0 == 6);
    CHECK(fake_hip_copies() - c0 == 1 + 2 * (1 + 1 + 5 + 10));                    // offsets; per range: points, masks, five lists up, ten arrays back
    CHECK(out.lists_untouched() && out.mask_count[0] == 0 && out.mask_count[(size_t)b.F * b.M - 1] == 0 && out.mask_count[(size_t)b.F * b.M] == 7);
    lpf_first_match_input dev = b.input(1, false);                                 // lent masks cost a range nothing: one range
    const long long l1 = fake_hip_launches();
    CHECK(lpf_first_match(c, b.pts.data(), b.frame_off.data(), b.F, 0, &dev, &o) == LPF_OK && fake_hip_launches() - l1 == 3);
}

int main()
{
    lpf_ctx *c = drive_begin();
    refusals(c);
    runs(c);
    chunks(c);
    lpf_destroy(c);
    return drive_finish("drive_first_match", true);
}
