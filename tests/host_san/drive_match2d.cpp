// drive_match2d.cpp -- drives lpf_match_2d's HOST side (lpf_api.hip compiled --offload-host-only against fake_hip.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: its refused arguments and their messages, host and device pointers, frames without
// detections or boxes, F = 0, and the loop over frame ranges (three frames of 256 x 20 000 pairs with five host matrices are 614 MB:
// one frame per range under the 256 MiB bound).  Kernel launches do nothing here (fake_hip.cpp): the launches and copies are counted,
// the values are checked on the GPU by tests/test_gpu_match2d.py.
#include "drive_common.h"
#include <cmath>

struct Batch {                    // F frames with the given detection and box counts
    std::vector<int32_t> det_off, box_off, front;
    std::vector<float> dets;
    std::vector<double> bbox2d;
    long long P = 0;
    Batch(const std::vector<int> &D, const std::vector<int> &B)
    {
        det_off.push_back(0); box_off.push_back(0);
        for (size_t f = 0; f < D.size(); ++f) {
            det_off.push_back(det_off.back() + D[f]);
            box_off.push_back(box_off.back() + B[f]);
            P += (long long)D[f] * B[f];
        }
        dets.assign((size_t)det_off.back() * 4, 1.0f);
        bbox2d.assign((size_t)box_off.back() * 4, 2.0);
        front.assign((size_t)box_off.back(), 8);
    }
    int F() const { return (int)det_off.size() - 1; }
    lpf_match2d_input input(int on_device) const
    {
        lpf_match2d_input in;
        memset(&in, 0, sizeof in);
        in.dets = dets.empty() ? nullptr : dets.data(); in.det_off = det_off.data();
        in.bbox2d = bbox2d.empty() ? nullptr : bbox2d.data(); in.front = front.empty() ? nullptr : front.data();
        in.box_off = box_off.data();
        in.on_device = on_device;
        in.min_iou = 0.25; in.w_iou = 0.5; in.w_center = 0.3; in.w_size = 0.2;
        return in;
    }
};

struct Out {
    std::vector<int32_t> best_box;
    std::vector<double> best_iou, mats[5];
    Out(const Batch &b, int nmat) : best_box((size_t)b.det_off.back(), 7), best_iou((size_t)b.det_off.back(), 7.0)
    {
        for (int m = 0; m < nmat; ++m) mats[m].assign((size_t)b.P, 7.0);
    }
    lpf_match2d_outputs outputs(int on_device, bool best = true)
    {
        lpf_match2d_outputs o;
        memset(&o, 0, sizeof o);
        if (best) { o.best_box = best_box.data(); o.best_iou = best_iou.data(); }
        double **slot[5] = {&o.iou, &o.center_score, &o.size_score, &o.total_score, &o.cost};
        for (int m = 0; m < 5; ++m) *slot[m] = mats[m].empty() ? nullptr : mats[m].data();
        o.on_device = on_device;
        return o;
    }
};

static void refusals(lpf_ctx *c)
{
    Batch b({3, 0, 2}, {4, 5, 0});
    Out out(b, 5);
    lpf_match2d_input in = b.input(0);
    lpf_match2d_outputs o = out.outputs(0);
    CHECK(lpf_match_2d(nullptr, 3, &in, &o) == LPF_ERR_ARG);
    CHECK(lpf_match_2d(c, 3, &in, &o) == LPF_OK);                     // no camera, masks or boxes are needed
    CHECK(lpf_match_2d(c, -1, &in, &o) == LPF_ERR_ARG && err_starts("match_2d: in="));
    CHECK(lpf_match_2d(c, 3, nullptr, &o) == LPF_ERR_ARG && lpf_match_2d(c, 3, &in, nullptr) == LPF_ERR_ARG);
    lpf_match2d_input x = in;
    x.det_off = nullptr;
    CHECK(lpf_match_2d(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("match_2d: det_off="));
    x = in; x.box_off = nullptr;
    CHECK(lpf_match_2d(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("match_2d: det_off="));
    std::vector<int32_t> bad = b.det_off;
    bad[2] = bad[1] - 1;
    x = in; x.det_off = bad.data();
    CHECK(lpf_match_2d(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("match_2d: det_off decreases at frame 1"));
    bad = b.box_off; bad[1] = bad[0] - 1;
    x = in; x.box_off = bad.data();
    CHECK(lpf_match_2d(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("match_2d: box_off decreases at frame 0"));
    bad = b.det_off; bad[0] = -1;
    x = in; x.det_off = bad.data();
    CHECK(lpf_match_2d(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("match_2d: det_off[0]=-1"));
    x = in; x.dets = nullptr;
    CHECK(lpf_match_2d(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("match_2d: dets="));
    x = in; x.bbox2d = nullptr;
    CHECK(lpf_match_2d(c, 3, &x, &o) == LPF_ERR_ARG);
    x = in; x.front = nullptr;
    CHECK(lpf_match_2d(c, 3, &x, &o) == LPF_ERR_ARG);
    x = in; x.min_iou = NAN;
    CHECK(lpf_match_2d(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("match_2d: min_iou=nan"));
    x = in; x.w_center = INFINITY;
    CHECK(lpf_match_2d(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("match_2d: min_iou=0.25 weights=0.5 inf 0.2 must be finite"));
    // F = 0; a batch without detections (no dets array); a batch without boxes (no box arrays); no output asked for
    CHECK(lpf_match_2d(c, 0, &in, &o) == LPF_OK);
    {
        Batch nd({0, 0}, {3, 4});
        Out no(nd, 5);
        lpf_match2d_input i2 = nd.input(0);
        lpf_match2d_outputs o2 = no.outputs(0);
        const long long l0 = fake_hip_launches();
        CHECK(i2.dets == nullptr && lpf_match_2d(c, 2, &i2, &o2) == LPF_OK && fake_hip_launches() == l0);
        Batch nb({3, 4}, {0, 0});
        Out no3(nb, 5);
        lpf_match2d_input i3 = nb.input(0);
        lpf_match2d_outputs o3 = no3.outputs(0);
        CHECK(i3.bbox2d == nullptr && i3.front == nullptr && lpf_match_2d(c, 2, &i3, &o3) == LPF_OK);
        CHECK(fake_hip_launches() == l0 + 1);                          // the detections still get their -1 / 0
        lpf_match2d_outputs none;
        memset(&none, 0, sizeof none);
        CHECK(lpf_match_2d(c, 3, &in, &none) == LPF_OK && fake_hip_launches() == l0 + 1);
    }
    // while a graph is captured the call is refused
    CHECK(lpf_graph_begin(c) == LPF_OK);
    CHECK(lpf_match_2d(c, 3, &in, &o) == LPF_ERR_STATE && err_starts("lpf_match_2d cannot be captured"));
    CHECK(lpf_match_2d(c, 3, &in, &o) == LPF_OK);                     // (the refusal abandoned the capture)
}

// host and device memory in every combination, float32 and float64 detections, each selection of outputs; then the range loop
static void runs(lpf_ctx *c)
{
    {
        Batch b({5, 0, 17, 300, 1}, {7, 3, 0, 600, 1});
        std::vector<double> d64(b.dets.size(), 1.0);
        for (int in_dev = 0; in_dev < 2; ++in_dev)
            for (int out_dev = 0; out_dev < 2; ++out_dev)
                for (int f64 = 0; f64 < 2; ++f64)
                    for (int nmat = 0; nmat <= 5; nmat += 5)
                        for (int best = 0; best < 2; ++best) {
                            if (!best && !nmat) continue;
                            Out out(b, nmat);
                            lpf_match2d_input in = b.input(in_dev);
                            if (f64) { in.dets = d64.data(); in.dets_f64 = 1; }
                            lpf_match2d_outputs o = out.outputs(out_dev, best != 0);
                            const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
                            CHECK(lpf_match_2d(c, b.F(), &in, &o) == LPF_OK);
                            CHECK(fake_hip_launches() - l0 == 1);                  // one range: one launch
                            const long long copies = 1 + (in_dev ? 0 : 3) + (out_dev ? 0 : 2 * best + nmat);    // the table; dets, bbox2d, front; outputs
                            CHECK(fake_hip_copies() - c0 == copies);
                        }
    }
    {
        Batch b({256, 256, 256, 2}, {20000, 20000, 20000, 5});            // 41 MB per matrix and frame: 205 MB per frame with all five
        Out out(b, 5);
        lpf_match2d_input in = b.input(0);
        lpf_match2d_outputs o = out.outputs(0);
        const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
        CHECK(lpf_match_2d(c, b.F(), &in, &o) == LPF_OK);
        CHECK(fake_hip_launches() - l0 == 3);                             // ranges {0}, {1}, {2, 3}
        CHECK(fake_hip_copies() - c0 == 1 + 3 * (3 + 7));
        lpf_match2d_outputs od = out.outputs(1);                          // device outputs: the staged inputs alone bound a range
        const long long l1 = fake_hip_launches();
        CHECK(lpf_match_2d(c, b.F(), &in, &od) == LPF_OK);
        CHECK(fake_hip_launches() - l1 == 1);
        lpf_match2d_input ind = b.input(1);                               // all on the device: one launch, only the table is copied
        const long long l2 = fake_hip_launches(), c2 = fake_hip_copies();
        CHECK(lpf_match_2d(c, b.F(), &ind, &od) == LPF_OK);
        CHECK(fake_hip_launches() - l2 == 1 && fake_hip_copies() - c2 == 1);
        int64_t st[8];
        CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK);
        CHECK(lpf_match_2d(c, b.F(), &ind, &od) == LPF_OK);
        CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK && st[0] == 0 && st[6] == 0 && st[2] == 1);      // no host wait, one ring upload
    }
}

int main()
{
    lpf_ctx *c = drive_begin();
    refusals(c);
    runs(c);
    lpf_destroy(c);
    return drive_finish("drive_match2d", true);
}
