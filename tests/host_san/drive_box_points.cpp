// drive_box_points.cpp -- drives lpf_box_points' HOST side (lpf_api.hip compiled --offload-host-only against fake_hip.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: its refused arguments and their messages, the state it needs (boxes in force, for the
// same number of frames), host and device memory for the points, the lists and the outputs in every combination, NULL outputs in every
// combination, LW = 0 and NULL labels, F = 0, a frame with n_valid = 0, a frame without boxes, the checks of host lists, and what goes
// back to a host caller (only a frame's first n_valid entries of first_box).  Kernel launches do nothing here (fake_hip.cpp): the
// launches and copies are counted, the values are checked on the GPU by tests/test_gpu_box_points.py.
#include "drive_common.h"

struct Batch {                    // F frames of N points, frame f with nv[f % size] valid points (every other point), B boxes per frame
    int F, N, LW;
    std::vector<float> pts;
    std::vector<int64_t> frame_off, valid_idx, n_valid;
    std::vector<uint32_t> labels;
    std::vector<int32_t> box_off;
    std::vector<double> corners;
    Batch(int F_, int N_, const std::vector<int> &nv, int LW_, int B) : F(F_), N(N_), LW(LW_)
    {
        frame_off.push_back(0); box_off.push_back(0);
        for (int f = 0; f < F; ++f) { frame_off.push_back(frame_off.back() + N); box_off.push_back(box_off.back() + B); }
        pts.assign((size_t)F * N * 4, 0.5f);
        valid_idx.assign((size_t)F * N, 0);
        for (int f = 0; f < F; ++f) {
            n_valid.push_back(nv[(size_t)f % nv.size()]);
            for (int e = 0; e < n_valid.back(); ++e) valid_idx[(size_t)f * N + e] = 2 * e;
        }
        labels.assign((size_t)F * N * (LW > 0 ? LW : 1), 1u);
        unit_cubes(corners, (size_t)F * B);
    }
    lpf_box_points_input input(int on_device) const
    {
        lpf_box_points_input in;
        memset(&in, 0, sizeof in);
        in.valid_idx = valid_idx.data(); in.n_valid = n_valid.data(); in.label_valid_words = labels.data();
        in.LW = LW; in.on_device = on_device;
        return in;
    }
    int set_boxes(lpf_ctx *c) const { return lpf_set_boxes(c, corners.empty() ? nullptr : corners.data(), box_off.data(), F, 1); }
};

struct Out {
    std::vector<int32_t> box_points, box_labelled, first_box;
    std::vector<int64_t> frame_counts;
    explicit Out(const Batch &b) : box_points((size_t)b.box_off.back() + 1, 7), box_labelled((size_t)b.box_off.back() + 1, 7),
                                   first_box((size_t)b.F * b.N + 1, 7), frame_counts((size_t)b.F * 4 + 1, 7) {}
    lpf_box_points_outputs outputs(int on_device, unsigned which = 15)
    {
        lpf_box_points_outputs o;
        memset(&o, 0, sizeof o);
        if (which & 1) o.box_points = box_points.data();
        if (which & 2) o.box_labelled = box_labelled.data();
        if (which & 4) o.first_box = first_box.data();
        if (which & 8) o.frame_counts = frame_counts.data();
        o.on_device = on_device;
        return o;
    }
};

static void refusals(lpf_ctx *c)
{
    Batch b(3, 100, {40, 0, 50}, 1, 2);
    Out out(b);
    lpf_box_points_input in = b.input(0);
    lpf_box_points_outputs o = out.outputs(0);
    const float *pts = b.pts.data();
    const int64_t *fo = b.frame_off.data();
    CHECK(lpf_box_points(nullptr, pts, fo, 3, 0, &in, &o) == LPF_ERR_ARG);
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &in, &o) == LPF_ERR_STATE && err_starts("box_points: no boxes in force"));
    CHECK(lpf_box_points(c, pts, fo, 0, 0, &in, &o) == LPF_OK);                   // F = 0 does nothing, with or without boxes
    CHECK(b.set_boxes(c) == LPF_OK);
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &in, &o) == LPF_OK);
    CHECK(lpf_box_points(c, pts, fo, 2, 0, &in, &o) == LPF_ERR_STATE && err_starts("boxes were set for 3 frames, box_points has 2"));
    CHECK(lpf_box_points(c, pts, fo, -1, 0, &in, &o) == LPF_ERR_ARG && err_starts("box_points: in="));
    CHECK(lpf_box_points(c, pts, fo, 3, 0, nullptr, &o) == LPF_ERR_ARG && lpf_box_points(c, pts, fo, 3, 0, &in, nullptr) == LPF_ERR_ARG);
    CHECK(lpf_box_points(c, pts, nullptr, 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("box_points: in="));
    CHECK(lpf_box_points(c, nullptr, fo, 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("box_points: pts is NULL"));
    lpf_box_points_input x = in;
    x.LW = -1;
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("box_points: LW=-1"));
    x.LW = LPF_MAX_MASKS_WIDE / 32 + 1;
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("box_points: LW=9"));
    x = in; x.valid_idx = nullptr;
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("box_points: valid_idx="));
    x = in; x.n_valid = nullptr;
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("box_points: valid_idx="));
    std::vector<int64_t> bad = b.frame_off;
    bad[2] = bad[1] - 1;
    CHECK(lpf_box_points(c, pts, bad.data(), 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("box_points: frame 1 has -1 points"));
    bad = b.frame_off; bad[0] = 1;
    CHECK(lpf_box_points(c, pts, bad.data(), 3, 0, &in, &o) == LPF_ERR_ARG && err_starts("box_points: frame_off[0] must be 0"));
    // the checks of host lists: n_valid within [0, N_f], indices within [0, N_f) and strictly ascending
    bad = b.n_valid; bad[1] = -1;
    x = in; x.n_valid = bad.data();
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("box_points: frame 1: n_valid=-1, the frame has 100 points"));
    bad = b.n_valid; bad[2] = 101;
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("box_points: frame 2: n_valid=101"));
    bad = b.valid_idx; bad[200 + 7] = 100;
    x = in; x.valid_idx = bad.data();
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("box_points: frame 2 entry 7: index 100, the frame has 100 points"));
    bad = b.valid_idx; bad[0] = -1;
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("box_points: frame 0 entry 0: index -1"));
    bad = b.valid_idx; bad[5] = bad[4];
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_ERR_ARG && err_starts("box_points: frame 0 entry 5: index 8 does not ascend"));
    bad = b.valid_idx; bad[45] = -9; bad[100] = 1000;                             // beyond a frame's n_valid nothing is looked at
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_OK);
    x.on_device = 1;                                                              // device lists are not checked
    bad[5] = bad[4];
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &x, &o) == LPF_OK);
    // while a graph is captured the call is refused
    CHECK(lpf_graph_begin(c) == LPF_OK);
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &in, &o) == LPF_ERR_STATE && err_starts("lpf_box_points cannot be captured"));
    CHECK(lpf_box_points(c, pts, fo, 3, 0, &in, &o) == LPF_OK);                   // (the refusal abandoned the capture)
}

// host and device memory in every combination, every selection of outputs; what a host caller gets back
static void runs(lpf_ctx *c)
{
    Batch b(3, 100, {40, 0, 50}, 2, 2);                                           // frame 1 has no valid point
    CHECK(b.set_boxes(c) == LPF_OK);
    {
        Out warm(b);                                                              // (the box tables are built by the first call)
        lpf_box_points_input in = b.input(0);
        lpf_box_points_outputs o = warm.outputs(0);
        CHECK(lpf_box_points(c, b.pts.data(), b.frame_off.data(), 3, 0, &in, &o) == LPF_OK);
    }
    for (int pts_dev = 0; pts_dev < 2; ++pts_dev)
        for (int in_dev = 0; in_dev < 2; ++in_dev)
            for (int out_dev = 0; out_dev < 2; ++out_dev)
                for (int labels = 0; labels < 3; ++labels)                        // label words; NULL labels; LW = 0
                    for (unsigned which = 0; which < 16; ++which) {
                        Out out(b);
                        lpf_box_points_input in = b.input(in_dev);
                        if (labels == 1) in.label_valid_words = nullptr;
                        if (labels == 2) in.LW = 0;
                        lpf_box_points_outputs o = out.outputs(out_dev, which);
                        const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
                        CHECK(lpf_box_points(c, b.pts.data(), b.frame_off.data(), 3, pts_dev, &in, &o) == LPF_OK);
                        CHECK(fake_hip_launches() - l0 == (which ? 1 : 0));       // one launch, none when nothing is asked for
                        long long copies = 0;
                        if (which) {
                            copies = 1 + (pts_dev ? 0 : 1) + (in_dev ? 0 : (labels ? 2 : 3));     // the frame table; the points; the lists
                            if (!out_dev) {
                                copies += ((which & 1) ? 1 : 0) + ((which & 2) ? 1 : 0) + ((which & 8) ? 1 : 0);
                                // first_box: the two frames with valid points, each by itself; with device lists up and back whole
                                if (which & 4) copies += 2;
                            }
                        }
                        CHECK(fake_hip_copies() - c0 == copies);
                        // entries beyond a frame's n_valid, and the slot behind every array, stay as they were
                        CHECK(out.first_box[45] == 7 && out.first_box[100] == 7 && out.first_box[199] == 7 && out.first_box[250] == 7);
                        CHECK(out.first_box[300] == 7 && out.box_points[6] == 7 && out.box_labelled[6] == 7 && out.frame_counts[12] == 7);
                        if (!out_dev && (which & 1)) CHECK(out.box_points[0] == 0 && out.box_points[5] == 0);    // (zeroed; the fake kernel adds nothing)
                        if (!out_dev && (which & 8)) CHECK(out.frame_counts[0] == 0 && out.frame_counts[11] == 0);
                    }
    {
        // frames without boxes, and a batch without points: still legal
        Batch nb(2, 10, {4, 5}, 1, 0);
        CHECK(nb.set_boxes(c) == LPF_OK);
        Out out(nb);
        lpf_box_points_input in = nb.input(0);
        lpf_box_points_outputs o = out.outputs(0);
        const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
        CHECK(lpf_box_points(c, nb.pts.data(), nb.frame_off.data(), 2, 0, &in, &o) == LPF_OK && fake_hip_launches() == l0 + 1);
        CHECK(fake_hip_copies() - c0 == 1 + 1 + 3 + 1 + 2);                       // table, points, lists; frame_counts and first_box per frame back
        CHECK(out.first_box[4] == 7 && out.first_box[9] == 7 && out.first_box[15] == 7 && out.first_box[20] == 7);
        Batch np(2, 0, {0}, 1, 1);
        CHECK(np.set_boxes(c) == LPF_OK);
        Out out2(np);
        lpf_box_points_input in2 = np.input(0);
        const int64_t none = 0;
        in2.valid_idx = &none;                                                    // (required even where no entry is read)
        lpf_box_points_outputs o2 = out2.outputs(0);
        CHECK(lpf_box_points(c, nullptr, np.frame_off.data(), 2, 0, &in2, &o2) == LPF_OK && fake_hip_launches() == l0 + 3);     // (its box tables' job, then the kernel)
        CHECK(out2.box_points[0] == 0 && out2.box_points[1] == 0 && out2.box_points[2] == 7 && out2.frame_counts[7] == 0);
    }
    {
        // everything on the device: no host wait, no blocking upload, one ring upload (the frame table) -- and the second call of the
        // shape allocates nothing (an allocation of a buffer in use would drain first: a host wait)
        Batch d(3, 100, {40, 0, 50}, 2, 2);
        CHECK(d.set_boxes(c) == LPF_OK);
        Out out(d);
        lpf_box_points_input in = d.input(1);
        lpf_box_points_outputs o = out.outputs(1);
        CHECK(lpf_box_points(c, d.pts.data(), d.frame_off.data(), 3, 1, &in, &o) == LPF_OK);
        int64_t st[8];
        CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK);
        const long long c0 = fake_hip_copies();
        CHECK(lpf_box_points(c, d.pts.data(), d.frame_off.data(), 3, 1, &in, &o) == LPF_OK);
        CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK && st[0] == 0 && st[1] == 0 && st[6] == 0 && st[2] == 1);
        CHECK(fake_hip_copies() - c0 == 1);
    }
}

int main()
{
    lpf_ctx *c = drive_begin();
    set_camera(c);
    refusals(c);
    runs(c);
    lpf_destroy(c);
    return drive_finish("drive_box_points", true);
}
