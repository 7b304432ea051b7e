// drive_inside.cpp -- drives lpf_inside_masks' HOST side (lpf_api.hip compiled --offload-host-only against fake_hip.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: its refused arguments and their messages, the state it needs (boxes in force, for the
// same number of frames), host and device memory for the points, the lists and the outputs in every combination, NULL outputs, M = 0,
// F = 0, a frame whose lists did not fit, and what goes back to a host caller (only the entries a frame lists).  Kernel launches do
// nothing here (fake_hip.cpp): the launches and copies are counted, the values are checked on the GPU by tests/test_gpu_inside.py.
#include "drive_common.h"

struct Batch {                    // F frames of N points, M cars per frame with the given list lengths, B boxes per frame
    int F, M;
    int64_t cap;
    std::vector<float> pts;
    std::vector<int64_t> frame_off, inst_idx, inst_off, best_cnt;
    std::vector<int32_t> best_box, box_off;
    std::vector<double> corners;
    Batch(int F_, int M_, int N, const std::vector<int> &len, int64_t cap_, int B) : F(F_), M(M_), cap(cap_)
    {
        frame_off.push_back(0); box_off.push_back(0);
        for (int f = 0; f < F; ++f) { frame_off.push_back(frame_off.back() + N); box_off.push_back(box_off.back() + B); }
        pts.assign((size_t)F * N * 4, 1.0f);
        inst_idx.assign((size_t)F * cap, 0);
        for (int f = 0; f < F; ++f) {
            inst_off.push_back(0);
            for (int m = 0; m < M; ++m) inst_off.push_back(inst_off.back() + len[(size_t)m % len.size()]);
        }
        best_box.assign((size_t)F * M, B > 0 ? 0 : -1);
        best_cnt.assign((size_t)F * M, 12);
        unit_cubes(corners, (size_t)F * B);
    }
    lpf_inside_input input(int on_device) const
    {
        lpf_inside_input in;
        memset(&in, 0, sizeof in);
        in.inst_idx = inst_idx.data(); in.inst_cap = cap; in.inst_off = inst_off.data();
        in.best_box = best_box.empty() ? nullptr : best_box.data(); in.best_cnt = best_cnt.empty() ? nullptr : best_cnt.data();
        in.M = M; in.min_points = 10; in.on_device = on_device;
        return in;
    }
    int set_boxes(lpf_ctx *c) const { return lpf_set_boxes(c, corners.empty() ? nullptr : corners.data(), box_off.data(), F, 1); }
};

struct Out {
    std::vector<uint8_t> inside;
    std::vector<int64_t> part_idx, n_inside;
    std::vector<float> part_xyz;
    std::vector<int32_t> matched;
    explicit Out(const Batch &b) : inside((size_t)b.F * b.cap, 7), part_idx((size_t)b.F * b.cap, 7), n_inside((size_t)b.F * b.M + 1, 7),
                                   part_xyz((size_t)b.F * b.cap * 3, 7.0f), matched((size_t)b.F * b.M + 1, 7) {}
    lpf_inside_outputs outputs(int on_device, unsigned which = 31)
    {
        lpf_inside_outputs o;
        memset(&o, 0, sizeof o);
        if (which & 1) o.inside = inside.data();
        if (which & 2) o.part_idx = part_idx.data();
        if (which & 4) o.part_xyz = part_xyz.data();
        if (which & 8) o.n_inside = n_inside.data();
        if (which & 16) o.matched = matched.data();
        o.on_device = on_device;
        return o;
    }
};

static void refusals(lpf_ctx *c)
{
    Batch b(3, 4, 100, {5, 0, 20, 3}, 64, 2);
    Out out(b);
    lpf_inside_input in = b.input(0);
    lpf_inside_outputs o = out.outputs(0);
    const float *pts = b.pts.data();
    const int64_t *fo = b.frame_off.data();
    CHECK(lpf_inside_masks(nullptr, pts, fo, 3, 0, &in, &o) == LPF_ERR_ARG);
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &in, &o) == LPF_ERR_STATE && err_starts("inside_masks: no boxes in force"));
    CHECK(lpf_inside_masks(c, pts, fo, 0, 0, &in, &o) == LPF_OK);                 // F = 0 does nothing, with or without boxes
    CHECK(b.set_boxes(c) == LPF_OK);
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &in, &o) == LPF_OK);
    CHECK(lpf_inside_masks(c, pts, fo, 2, 0, &in, &o) == LPF_ERR_STATE && err_starts("boxes were set for 3 frames, inside_masks has 2"));
    CHECK(lpf_inside_masks(c, pts, fo, -1, 0, &in, &o) == LPF_ERR_ARG && err_starts("inside_masks: in="));
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, nullptr, &o) == LPF_ERR_ARG && lpf_inside_masks(c, pts, fo, 3, 0, &in, nullptr) == LPF_ERR_ARG);
    CHECK(lpf_inside_masks(c, pts, nullptr, 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("inside_masks: in="));
    CHECK(lpf_inside_masks(c, nullptr, fo, 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("inside_masks: pts is NULL"));
    lpf_inside_input x = in;
    x.M = -1;
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("inside_masks: M=-1"));
    x.M = LPF_MAX_MASKS_WIDE + 1;
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("inside_masks: M=257"));
    x = in; x.inst_cap = -1;
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("inside_masks: inst_cap=-1"));
    x = in; x.min_points = -2;
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("inside_masks: inst_cap=64 min_points=-2"));
    x = in; x.inst_off = nullptr;
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("inside_masks: inst_idx="));
    x = in; x.best_box = nullptr;
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG);
    x = in; x.best_cnt = nullptr;
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG);
    x = in; x.inst_idx = nullptr;
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG);
    std::vector<int64_t> bad = b.frame_off;
    bad[2] = bad[1] - 1;
    CHECK(lpf_inside_masks(c, pts, bad.data(), 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("inside_masks: frame 1 has -1 points"));
    bad = b.inst_off; bad[5 + 2] = bad[5 + 1] - 1;
    x = in; x.inst_off = bad.data();
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("inside_masks: frame 1: inst_off decreases at car 1"));
    bad = b.inst_off; bad[10] = -3;
    x = in; x.inst_off = bad.data();
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("inside_masks: frame 2: inst_off[0]=-3"));
    std::vector<int32_t> bb = b.best_box;
    bb[6] = 2;
    x = in; x.best_box = bb.data();
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("inside_masks: frame 1 car 2: best_box=2, the frame has 2 boxes"));
    bb[6] = -5;                                                                  // any negative box is "none"
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_OK);
    std::vector<int64_t> bc = b.best_cnt;
    bc[1] = -1;
    x = in; x.best_cnt = bc.data();
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("inside_masks: frame 0 car 1: best_cnt=-1"));
    // while a graph is captured the call is refused
    CHECK(lpf_graph_begin(c) == LPF_OK);
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &in, &o) == LPF_ERR_STATE && err_starts("lpf_inside_masks cannot be captured"));
    CHECK(lpf_inside_masks(c, pts, fo, 3, 0, &in, &o) == LPF_OK);                 // (the refusal abandoned the capture)
}

// host and device memory in every combination, every selection of outputs; what a host caller gets back
static void runs(lpf_ctx *c)
{
    Batch b(3, 4, 100, {5, 0, 20, 3}, 64, 2);                                     // 28 entries listed per frame, room for 64
    CHECK(b.set_boxes(c) == LPF_OK);
    {
        Out warm(b);                                                              // (the box tables are built by the first call)
        lpf_inside_input in = b.input(0);
        lpf_inside_outputs o = warm.outputs(0);
        CHECK(lpf_inside_masks(c, b.pts.data(), b.frame_off.data(), 3, 0, &in, &o) == LPF_OK);
    }
    for (int pts_dev = 0; pts_dev < 2; ++pts_dev)
        for (int in_dev = 0; in_dev < 2; ++in_dev)
            for (int out_dev = 0; out_dev < 2; ++out_dev)
                for (unsigned which = 0; which < 32; ++which) {
                    Out out(b);
                    lpf_inside_input in = b.input(in_dev);
                    lpf_inside_outputs o = out.outputs(out_dev, which);
                    const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
                    CHECK(lpf_inside_masks(c, b.pts.data(), b.frame_off.data(), 3, pts_dev, &in, &o) == LPF_OK);
                    CHECK(fake_hip_launches() - l0 == (which ? 1 : 0));           // one launch, none when nothing is asked for
                    const int rows = ((which & 1) ? 1 : 0) + ((which & 2) ? 1 : 0) + ((which & 4) ? 1 : 0);
                    long long copies = 1 + (pts_dev ? 0 : 1) + (in_dev ? 0 : 4);  // the frame table; the points; the four list arrays
                    if (!out_dev) copies += ((which & 8) ? 1 : 0) + ((which & 16) ? 1 : 0) + 3 * rows + ((in_dev && rows) ? 1 : 0);
                    CHECK(fake_hip_copies() - c0 == copies);                      // per frame and row array one copy back; device lists: their offsets first
                    if (!out_dev) {                                               // entries beyond a frame's lists stay as they were
                        for (int f = 0; f < 3; ++f)
                            for (int64_t e = 28; e < 64; ++e) {
                                CHECK(out.inside[(size_t)f * 64 + e] == 7 && out.part_idx[(size_t)f * 64 + e] == 7);
                                CHECK(out.part_xyz[((size_t)f * 64 + e) * 3 + 2] == 7.0f);
                            }
                        CHECK(out.n_inside[12] == 7 && out.matched[12] == 7);
                    }
                }
    {
        // a frame whose lists did not fit (inst_off[M] > inst_cap) is skipped: nothing of its rows comes back
        Batch v(2, 3, 50, {30, 30, 30}, 64, 1);
        CHECK(v.set_boxes(c) == LPF_OK);
        for (int m = 1; m <= 3; ++m) v.inst_off[(size_t)m] = 10 * m;              // frame 0 fits (30 entries), frame 1 lists 90 > 64
        Out out(v);
        lpf_inside_input in = v.input(0);
        lpf_inside_outputs o = out.outputs(0);
        const long long c0 = fake_hip_copies();
        CHECK(lpf_inside_masks(c, v.pts.data(), v.frame_off.data(), 2, 0, &in, &o) == LPF_OK);
        CHECK(fake_hip_copies() - c0 == 1 + 1 + 4 + 2 + 3);
        CHECK(out.inside[64] == 7 && out.part_idx[64 + 10] == 7 && out.inside[30] == 7 && out.inside[29] != 7);
    }
    {
        // M = 0: nothing to write, nothing launched; frames without boxes: every car unmatched, still one launch
        Batch z(2, 0, 10, {0}, 0, 1);
        CHECK(z.set_boxes(c) == LPF_OK);
        Out out(z);
        lpf_inside_input in = z.input(0);
        in.inst_idx = nullptr;
        lpf_inside_outputs o = out.outputs(0);
        const long long l0 = fake_hip_launches();
        CHECK(lpf_inside_masks(c, z.pts.data(), z.frame_off.data(), 2, 0, &in, &o) == LPF_OK && fake_hip_launches() == l0);
        Batch nb(2, 2, 10, {4, 4}, 8, 0);
        CHECK(nb.set_boxes(c) == LPF_OK);
        Out out2(nb);
        lpf_inside_input in2 = nb.input(0);
        lpf_inside_outputs o2 = out2.outputs(0);
        CHECK(lpf_inside_masks(c, nb.pts.data(), nb.frame_off.data(), 2, 0, &in2, &o2) == LPF_OK && fake_hip_launches() == l0 + 1);
    }
    {
        // everything on the device: no host wait, one ring upload (the frame table)
        Batch d(3, 4, 100, {5, 0, 20, 3}, 64, 2);
        CHECK(d.set_boxes(c) == LPF_OK);
        Out out(d);
        lpf_inside_input in = d.input(1);
        lpf_inside_outputs o = out.outputs(1);
        CHECK(lpf_inside_masks(c, d.pts.data(), d.frame_off.data(), 3, 1, &in, &o) == LPF_OK);
        int64_t st[8];
        CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK);
        CHECK(lpf_inside_masks(c, d.pts.data(), d.frame_off.data(), 3, 1, &in, &o) == LPF_OK);
        CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK && st[0] == 0 && st[6] == 0 && st[2] == 1);
    }
}

int main()
{
    lpf_ctx *c = drive_begin();
    set_camera(c);
    refusals(c);
    runs(c);
    lpf_destroy(c);
    return drive_finish("drive_inside", true);
}
