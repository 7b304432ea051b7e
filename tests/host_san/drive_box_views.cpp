// drive_box_views.cpp -- drives lpf_box_views' HOST side (lpf_api.hip compiled --offload-host-only against fake_hip.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: its refused arguments and their messages, host and device pointers, frames without
// boxes, F = 0, every selection of outputs, and the loop over frame ranges (three frames of 400 000 boxes with host corners in and
// host corners_velo out are 154 MB each: one frame per range under the 256 MiB bound).  Kernel launches do nothing here
// (fake_hip.cpp): the launches and copies are counted, the values are checked on the GPU by tests/test_gpu_box_views.py.
#include "drive_common.h"
#include <cmath>

struct Batch {                    // F frames with the given box counts
    std::vector<int32_t> box_off;
    std::vector<double> corners;
    explicit Batch(const std::vector<int> &B)
    {
        box_off.push_back(0);
        for (int b : B) box_off.push_back(box_off.back() + b);
        corners.assign((size_t)box_off.back() * 24, 1.0);
    }
    int F() const { return (int)box_off.size() - 1; }
    size_t boxes() const { return (size_t)box_off.back(); }
    lpf_box_views_input input(int on_device) const
    {
        lpf_box_views_input in;
        memset(&in, 0, sizeof in);
        in.corners_cam0 = corners.empty() ? nullptr : corners.data();
        in.box_off = box_off.data();
        in.T_cam_to_velo = IDENT;
        in.on_device = on_device;
        in.min_points_in_view = 4; in.depth_lo = 0.1; in.depth_hi = 100.0; in.min_area = 100.0;
        return in;
    }
};

enum { KEEP = 1, REASON = 2, IN_VIEW = 4, NEAR = 8, AVG = 16, NEAR_BB = 32, FRONT = 64, BB = 128, FRONT_AVG = 256, KEPT_POS = 512,
       COUNTS = 1024, VELO = 2048, EVERYTHING = 4095 };

struct Out {
    std::vector<uint8_t> keep;
    std::vector<int32_t> i32[6];          // reason, in_view, near, front, kept_pos, frame_counts
    std::vector<double> f64[5];           // avg_depth, near_bbox2d, bbox2d, front_avg_depth, corners_velo
    Out(const Batch &b, int mask)
    {
        const size_t n = b.boxes();
        if (mask & KEEP) keep.assign(n + 1, 7);
        const int im[6] = {REASON, IN_VIEW, NEAR, FRONT, KEPT_POS, COUNTS};
        for (int k = 0; k < 6; ++k)
            if (mask & im[k]) i32[k].assign((k == 5 ? (size_t)b.F() * 6 : n) + 1, 7);
        const int fm[5] = {AVG, NEAR_BB, BB, FRONT_AVG, VELO};
        const size_t fw[5] = {1, 4, 4, 1, 24};
        for (int k = 0; k < 5; ++k)
            if (mask & fm[k]) f64[k].assign(n * fw[k] + 1, 7.0);
    }
    lpf_box_views_outputs outputs(int on_device)
    {
        lpf_box_views_outputs o;
        memset(&o, 0, sizeof o);
        auto p = [](auto &v) { return v.empty() ? nullptr : v.data(); };
        o.keep = p(keep);
        o.reason = p(i32[0]); o.corners_in_view = p(i32[1]); o.corners_near = p(i32[2]); o.front = p(i32[3]); o.kept_pos = p(i32[4]);
        o.frame_counts = p(i32[5]);
        o.avg_depth = p(f64[0]); o.near_bbox2d = p(f64[1]); o.bbox2d = p(f64[2]); o.front_avg_depth = p(f64[3]); o.corners_velo = p(f64[4]);
        o.on_device = on_device;
        return o;
    }
};

static int bits(int m) { int n = 0; for (; m; m &= m - 1) ++n; return n; }

static void refusals(lpf_ctx *c)
{
    Batch b({3, 0, 2});
    Out out(b, EVERYTHING);
    lpf_box_views_input in = b.input(0);
    lpf_box_views_outputs o = out.outputs(0);
    CHECK(lpf_box_views(nullptr, 3, &in, &o) == LPF_ERR_ARG);
    CHECK(lpf_box_views(c, 3, &in, &o) == LPF_ERR_STATE && err_starts("lpf_set_camera has not been called"));
    const double K[9] = {552.5, 0, 682.0, 0, 552.5, 238.7, 0, 0, 1};
    CHECK(lpf_set_camera(c, IDENT, K, 1408, 376, 0.0, 50.0) == LPF_OK);
    CHECK(lpf_box_views(c, 3, &in, &o) == LPF_OK);
    CHECK(lpf_box_views(c, -1, &in, &o) == LPF_ERR_ARG && err_starts("box_views: in="));
    CHECK(lpf_box_views(c, 3, nullptr, &o) == LPF_ERR_ARG && lpf_box_views(c, 3, &in, nullptr) == LPF_ERR_ARG);
    lpf_box_views_input x = in;
    x.box_off = nullptr;
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("box_views: box_off="));
    std::vector<int32_t> bad = b.box_off;
    bad[2] = bad[1] - 1;
    x = in; x.box_off = bad.data();
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("box_views: box_off decreases at frame 1"));
    bad = b.box_off; bad[0] = -1;
    x = in; x.box_off = bad.data();
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("box_views: box_off[0]=-1"));
    x = in; x.corners_cam0 = nullptr;
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("box_views: corners_cam0="));
    x = in; x.T_cam_to_velo = nullptr;
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("box_views: T_cam_to_velo="));
    {
        Out few(b, KEEP | COUNTS);                                      // without corners_velo the transform is not needed
        lpf_box_views_outputs o2 = few.outputs(0);
        CHECK(lpf_box_views(c, 3, &x, &o2) == LPF_OK);
    }
    x = in; x.depth_lo = NAN;
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("box_views: depth_lo=nan"));
    x = in; x.depth_hi = INFINITY;
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("box_views: depth_lo=0.1 depth_hi=inf min_area=100 must be finite"));
    x = in; x.min_area = -INFINITY;
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_ERR_ARG);
    x = in; x.min_points_in_view = 9;
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("box_views: min_points_in_view=9"));
    x = in; x.min_points_in_view = -1;
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("box_views: min_points_in_view=-1"));
    x = in; x.min_points_in_view = 0;
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_OK);
    x.min_points_in_view = 8;
    CHECK(lpf_box_views(c, 3, &x, &o) == LPF_OK);
    // F = 0; a batch without boxes (no corners): the counts are still written; no output asked for
    const long long l0 = fake_hip_launches();
    CHECK(lpf_box_views(c, 0, &in, &o) == LPF_OK && fake_hip_launches() == l0);
    {
        Batch nb({0, 0});
        Out no(nb, EVERYTHING);
        lpf_box_views_input i2 = nb.input(0);
        lpf_box_views_outputs o2 = no.outputs(0);
        CHECK(i2.corners_cam0 == nullptr && lpf_box_views(c, 2, &i2, &o2) == LPF_OK && fake_hip_launches() == l0 + 1);
        Out nc(nb, EVERYTHING & ~COUNTS);
        lpf_box_views_outputs o3 = nc.outputs(0);
        CHECK(lpf_box_views(c, 2, &i2, &o3) == LPF_OK && fake_hip_launches() == l0 + 1);        // nothing to write
        lpf_box_views_outputs none;
        memset(&none, 0, sizeof none);
        CHECK(lpf_box_views(c, 3, &in, &none) == LPF_OK && fake_hip_launches() == l0 + 1);
    }
    // while a graph is captured the call is refused
    CHECK(lpf_graph_begin(c) == LPF_OK);
    CHECK(lpf_box_views(c, 3, &in, &o) == LPF_ERR_STATE && err_starts("lpf_box_views cannot be captured"));
    CHECK(lpf_box_views(c, 3, &in, &o) == LPF_OK);                     // (the refusal abandoned the capture)
}

// host and device memory in every combination, each selection of outputs; then the range loop
static void runs(lpf_ctx *c)
{
    {
        Batch b({5, 0, 17, 314, 1, 0});
        const int masks[] = {EVERYTHING, KEEP, COUNTS, KEPT_POS | COUNTS, VELO, AVG | FRONT_AVG, BB | FRONT, NEAR_BB | IN_VIEW | NEAR | REASON};
        for (int in_dev = 0; in_dev < 2; ++in_dev)
            for (int out_dev = 0; out_dev < 2; ++out_dev)
                for (int m : masks) {
                    Out out(b, m);
                    lpf_box_views_input in = b.input(in_dev);
                    lpf_box_views_outputs o = out.outputs(out_dev);
                    const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
                    CHECK(lpf_box_views(c, b.F(), &in, &o) == LPF_OK);
                    CHECK(fake_hip_launches() - l0 == 1);                      // one range: one launch
                    const long long copies = 1 + (in_dev ? 0 : 1) + (out_dev ? 0 : bits(m));    // the table; corners; outputs
                    CHECK(fake_hip_copies() - c0 == copies);
                }
    }
    {
        Batch b({400000, 400000, 400000, 5});                             // 77 MB of corners per frame, and as much of corners_velo
        Out out(b, KEEP | VELO);
        lpf_box_views_input in = b.input(0);
        lpf_box_views_outputs o = out.outputs(0);
        const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
        CHECK(lpf_box_views(c, b.F(), &in, &o) == LPF_OK);
        CHECK(fake_hip_launches() - l0 == 3);                             // ranges {0}, {1}, {2, 3}
        CHECK(fake_hip_copies() - c0 == 1 + 3 * (1 + 2));
        lpf_box_views_outputs od = out.outputs(1);                        // device outputs: the staged corners alone bound a range
        const long long l1 = fake_hip_launches();
        CHECK(lpf_box_views(c, b.F(), &in, &od) == LPF_OK);
        CHECK(fake_hip_launches() - l1 == 1);
        lpf_box_views_input ind = b.input(1);                             // all on the device: one launch, only the table is copied
        const long long l2 = fake_hip_launches(), c2 = fake_hip_copies();
        CHECK(lpf_box_views(c, b.F(), &ind, &od) == LPF_OK);
        CHECK(fake_hip_launches() - l2 == 1 && fake_hip_copies() - c2 == 1);
        int64_t st[8];
        CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK);
        CHECK(lpf_box_views(c, b.F(), &ind, &od) == LPF_OK);
        CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK && st[0] == 0 && st[6] == 0 && st[2] == 1);      // no host wait, one ring upload
    }
}

int main()
{
    lpf_ctx *c = drive_begin();
    refusals(c);
    runs(c);
    lpf_destroy(c);
    return drive_finish("drive_box_views", true);
}
