// drive_assign.cpp -- drives the HOST side of lpf_assign_costs and lpf_assign_2d (lpf_api.hip compiled --offload-host-only against
// fake_hip.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: their refused arguments and their messages, host and device
// pointers, frames without rows or columns, F = 0, every selection of outputs, the loop over frame ranges (three frames of 1024 x 20 000
// pairs are 164 MB of scratch each: one frame per range under the 256 MiB bound) and no allocation on a second call of a shape.  Kernel
// launches do nothing here (fake_hip.cpp): the launches and copies are counted, the values are checked on the GPU by
// tests/test_gpu_assign.py.
#include "drive_common.h"
#include <cmath>

struct Batch {                    // F frames with the given row / detection and column / box counts
    std::vector<int32_t> det_off, box_off, front;
    std::vector<float> dets;
    std::vector<double> bbox2d, cost;
    long long P = 0;
    Batch(const std::vector<int> &D, const std::vector<int> &B, bool with_cost = true)
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
        if (with_cost) cost.assign((size_t)P, 0.5);
    }
    int F() const { return (int)det_off.size() - 1; }
    lpf_assign_input costs(int on_device, bool with_front = true) const
    {
        lpf_assign_input in;
        memset(&in, 0, sizeof in);
        in.cost = cost.empty() ? nullptr : cost.data();
        in.det_off = det_off.data(); in.box_off = box_off.data();
        in.front = with_front && !front.empty() ? front.data() : nullptr;
        in.on_device = on_device;
        return in;
    }
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

enum { COL = 1, STATUS = 2, IOU = 4, CENTER = 8, SIZE = 16, TOTAL = 32, ACCEPTED = 64, EVERYTHING = 127 };

struct Out {
    std::vector<int32_t> col, status, accepted;
    std::vector<double> f64[4];
    Out(const Batch &b, int mask)
    {
        const size_t n = (size_t)b.det_off.back();
        if (mask & COL) col.assign(n + 1, 7);
        if (mask & STATUS) status.assign((size_t)b.F() + 1, 7);
        if (mask & ACCEPTED) accepted.assign(n + 1, 7);
        const int fm[4] = {IOU, CENTER, SIZE, TOTAL};
        for (int k = 0; k < 4; ++k)
            if (mask & fm[k]) f64[k].assign(n + 1, 7.0);
    }
    lpf_assign_outputs costs(int on_device)
    {
        lpf_assign_outputs o;
        memset(&o, 0, sizeof o);
        o.col_of_row = col.empty() ? nullptr : col.data();
        o.status = status.empty() ? nullptr : status.data();
        o.on_device = on_device;
        return o;
    }
    lpf_assign2d_outputs outputs(int on_device)
    {
        lpf_assign2d_outputs o;
        memset(&o, 0, sizeof o);
        auto p = [](auto &v) { return v.empty() ? nullptr : v.data(); };
        o.box_of_det = p(col); o.status = p(status); o.accepted = p(accepted);
        o.iou = p(f64[0]); o.center_score = p(f64[1]); o.size_score = p(f64[2]); o.total_score = p(f64[3]);
        o.on_device = on_device;
        return o;
    }
};

static int bits(int m) { int n = 0; for (; m; m &= m - 1) ++n; return n; }
static const lpf_assign2d_params V5 = {0.3, 0.15};

static void refusals(lpf_ctx *c)
{
    Batch b({3, 0, 2}, {4, 5, 0});
    Out out(b, EVERYTHING);
    lpf_assign_input in = b.costs(0);
    lpf_assign_outputs o = out.costs(0);
    lpf_match2d_input in2 = b.input(0);
    lpf_assign2d_outputs o2 = out.outputs(0);
    CHECK(lpf_assign_costs(nullptr, 3, &in, &o) == LPF_ERR_ARG && lpf_assign_2d(nullptr, 3, &in2, &V5, &o2) == LPF_ERR_ARG);
    CHECK(lpf_assign_costs(c, 3, &in, &o) == LPF_OK);                  // no camera, masks or boxes are needed
    CHECK(lpf_assign_2d(c, 3, &in2, &V5, &o2) == LPF_OK);
    CHECK(lpf_assign_costs(c, -1, &in, &o) == LPF_ERR_ARG && err_starts("assign_costs: in="));
    CHECK(lpf_assign_costs(c, 3, nullptr, &o) == LPF_ERR_ARG && lpf_assign_costs(c, 3, &in, nullptr) == LPF_ERR_ARG);
    CHECK(lpf_assign_2d(c, -1, &in2, &V5, &o2) == LPF_ERR_ARG && err_starts("assign_2d: in="));
    CHECK(lpf_assign_2d(c, 3, nullptr, &V5, &o2) == LPF_ERR_ARG && lpf_assign_2d(c, 3, &in2, nullptr, &o2) == LPF_ERR_ARG &&
          lpf_assign_2d(c, 3, &in2, &V5, nullptr) == LPF_ERR_ARG);
    lpf_assign_input x = in;
    x.det_off = nullptr;
    CHECK(lpf_assign_costs(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("assign_costs: det_off="));
    x = in; x.box_off = nullptr;
    CHECK(lpf_assign_costs(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("assign_costs: det_off="));
    std::vector<int32_t> bad = b.det_off;
    bad[2] = bad[1] - 1;
    x = in; x.det_off = bad.data();
    CHECK(lpf_assign_costs(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("assign_costs: det_off decreases at frame 1"));
    bad = b.box_off; bad[1] = bad[0] - 1;
    x = in; x.box_off = bad.data();
    CHECK(lpf_assign_costs(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("assign_costs: box_off decreases at frame 0"));
    bad = b.det_off; bad[0] = -1;
    x = in; x.det_off = bad.data();
    CHECK(lpf_assign_costs(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("assign_costs: det_off[0]=-1"));
    x = in; x.cost = nullptr;
    CHECK(lpf_assign_costs(c, 3, &x, &o) == LPF_ERR_ARG && err_starts("assign_costs: cost="));
    x = in; x.front = nullptr;
    CHECK(lpf_assign_costs(c, 3, &x, &o) == LPF_OK);                   // no front: every column is live
    lpf_match2d_input y = in2;
    y.det_off = nullptr;
    CHECK(lpf_assign_2d(c, 3, &y, &V5, &o2) == LPF_ERR_ARG && err_starts("assign_2d: det_off="));
    bad = b.det_off; bad[3] = bad[2] - 1;
    y = in2; y.det_off = bad.data();
    CHECK(lpf_assign_2d(c, 3, &y, &V5, &o2) == LPF_ERR_ARG && err_starts("assign_2d: det_off decreases at frame 2"));
    y = in2; y.dets = nullptr;
    CHECK(lpf_assign_2d(c, 3, &y, &V5, &o2) == LPF_ERR_ARG && err_starts("assign_2d: dets="));
    y = in2; y.bbox2d = nullptr;
    CHECK(lpf_assign_2d(c, 3, &y, &V5, &o2) == LPF_ERR_ARG);
    y = in2; y.front = nullptr;
    CHECK(lpf_assign_2d(c, 3, &y, &V5, &o2) == LPF_ERR_ARG);
    y = in2; y.w_center = INFINITY;
    CHECK(lpf_assign_2d(c, 3, &y, &V5, &o2) == LPF_ERR_ARG && err_starts("assign_2d: weights=0.5 inf 0.2 must be finite"));
    y = in2; y.min_iou = NAN;                                          // (not used by this call)
    CHECK(lpf_assign_2d(c, 3, &y, &V5, &o2) == LPF_OK);
    lpf_assign2d_params q = V5;
    q.min_iou_threshold = NAN;
    CHECK(lpf_assign_2d(c, 3, &in2, &q, &o2) == LPF_ERR_ARG && err_starts("assign_2d: min_score_threshold=0.3 min_iou_threshold=nan"));
    // the cap: rows, and live columns where the host can count them
    {
        Batch big({2, 1025}, {3, 4});
        Out bo(big, COL | STATUS);
        lpf_assign_input bi = big.costs(0);
        lpf_assign_outputs bq = bo.costs(0);
        CHECK(lpf_assign_costs(c, 2, &bi, &bq) == LPF_ERR_ARG &&
              err_starts("assign_costs: frame 1: 1025 rows and 4 live columns, a frame takes at most LPF_ASSIGN_MAX = 1024 of either"));
        lpf_match2d_input bi2 = big.input(1);
        lpf_assign2d_outputs bq2 = bo.outputs(1);
        CHECK(lpf_assign_2d(c, 2, &bi2, &V5, &bq2) == LPF_ERR_ARG && err_starts("assign_2d: frame 1: 1025 rows"));
        Batch wide({4}, {1025});
        Out wo(wide, COL | STATUS);
        lpf_assign_input wi = wide.costs(0);
        lpf_assign_outputs wq = wo.costs(0);
        CHECK(lpf_assign_costs(c, 1, &wi, &wq) == LPF_ERR_ARG && err_starts("assign_costs: frame 0: 4 rows and 1025 live columns"));
        wide.front[7] = 0;                                             // one column without a projection: 1024 live ones fit
        CHECK(lpf_assign_costs(c, 1, &wi, &wq) == LPF_OK);
        wi.on_device = 1;                                              // (front in device memory is not counted: every column may be live)
        CHECK(lpf_assign_costs(c, 1, &wi, &wq) == LPF_ERR_ARG && err_starts("assign_costs: frame 0: 4 rows and 1025 live columns"));
    }
    // F = 0; frames without rows (no cost, no dets); frames without columns; no output asked for
    const long long l0 = fake_hip_launches();
    CHECK(lpf_assign_costs(c, 0, &in, &o) == LPF_OK && lpf_assign_2d(c, 0, &in2, &V5, &o2) == LPF_OK && fake_hip_launches() == l0);
    {
        Batch nd({0, 0}, {3, 4});
        Out no(nd, EVERYTHING);
        lpf_assign_input i1 = nd.costs(0);
        lpf_assign_outputs o1 = no.costs(0);
        CHECK(i1.cost == nullptr && lpf_assign_costs(c, 2, &i1, &o1) == LPF_OK && no.status[0] == 0 && no.status[1] == 0 && no.status[2] == 7);
        lpf_match2d_input i2 = nd.input(0);
        lpf_assign2d_outputs q2 = no.outputs(0);
        CHECK(i2.dets == nullptr && lpf_assign_2d(c, 2, &i2, &V5, &q2) == LPF_OK);
        Batch nb({3, 4}, {0, 0});
        Out no3(nb, EVERYTHING);
        lpf_match2d_input i3 = nb.input(0);
        lpf_assign2d_outputs q3 = no3.outputs(0);
        CHECK(i3.bbox2d == nullptr && i3.front == nullptr && lpf_assign_2d(c, 2, &i3, &V5, &q3) == LPF_OK && no3.status[1] == 0);
        lpf_assign_input i4 = nb.costs(0);
        lpf_assign_outputs o4 = no3.costs(0);
        CHECK(i4.cost == nullptr && lpf_assign_costs(c, 2, &i4, &o4) == LPF_OK);
        lpf_assign_outputs none;
        memset(&none, 0, sizeof none);
        CHECK(lpf_assign_costs(c, 3, &in, &none) == LPF_OK);           // the call keeps its own col_of_row and status
        lpf_assign2d_outputs none2;
        memset(&none2, 0, sizeof none2);
        CHECK(lpf_assign_2d(c, 3, &in2, &V5, &none2) == LPF_OK);
    }
    // while a graph is captured the calls are refused
    CHECK(lpf_graph_begin(c) == LPF_OK);
    CHECK(lpf_assign_costs(c, 3, &in, &o) == LPF_ERR_STATE && err_starts("lpf_assign_costs cannot be captured"));
    CHECK(lpf_assign_costs(c, 3, &in, &o) == LPF_OK);                  // (the refusal abandoned the capture)
    CHECK(lpf_graph_begin(c) == LPF_OK);
    CHECK(lpf_assign_2d(c, 3, &in2, &V5, &o2) == LPF_ERR_STATE && err_starts("lpf_assign_2d cannot be captured"));
    CHECK(lpf_assign_2d(c, 3, &in2, &V5, &o2) == LPF_OK);
}

// host and device memory in every combination, float32 and float64 detections, each selection of outputs; then the range loop
static void runs(lpf_ctx *c)
{
    {
        Batch b({5, 0, 17, 300, 1}, {7, 3, 0, 600, 1});
        std::vector<double> d64(b.dets.size(), 1.0);
        const int masks[] = {EVERYTHING, COL, STATUS, COL | STATUS, IOU | TOTAL, ACCEPTED, CENTER | SIZE | STATUS};
        for (int in_dev = 0; in_dev < 2; ++in_dev)
            for (int out_dev = 0; out_dev < 2; ++out_dev)
                for (int m : masks) {
                    Out out(b, m);
                    for (int f64 = 0; f64 < 2; ++f64) {
                        lpf_match2d_input in = b.input(in_dev);
                        if (f64) { in.dets = d64.data(); in.dets_f64 = 1; }
                        lpf_assign2d_outputs o = out.outputs(out_dev);
                        const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
                        CHECK(lpf_assign_2d(c, b.F(), &in, &V5, &o) == LPF_OK);
                        CHECK(fake_hip_launches() - l0 == 2 + ((m & ~(COL | STATUS)) ? 1 : 0));      // one range: pack, solve, (finish)
                        // the table; dets, bbox2d, front; outputs (the status memset is no copy)
                        CHECK(fake_hip_copies() - c0 == 1 + (in_dev ? 0 : 3) + (out_dev ? 0 : bits(m)));
                    }
                    if (m & ~(COL | STATUS)) continue;
                    for (int with_front = 0; with_front < 2; ++with_front) {
                        lpf_assign_input in = b.costs(in_dev, with_front != 0);
                        lpf_assign_outputs o = out.costs(out_dev);
                        const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
                        CHECK(lpf_assign_costs(c, b.F(), &in, &o) == LPF_OK);
                        CHECK(fake_hip_launches() - l0 == 2);
                        CHECK(fake_hip_copies() - c0 == 1 + (in_dev ? 0 : 1 + with_front) + (out_dev ? 0 : bits(m)));
                    }
                }
    }
    {
        Batch b({1024, 1024, 1024, 2}, {20000, 20000, 20000, 5}, false);   // 164 MB of scratch per frame
        for (size_t j = 0; j < b.front.size(); ++j) b.front[j] = j % 20 == 0 ? 8 : 0;      // 1000 live columns of 20 000
        Out out(b, EVERYTHING);
        lpf_match2d_input in = b.input(0);
        lpf_assign2d_outputs o = out.outputs(0);
        const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
        CHECK(lpf_assign_2d(c, b.F(), &in, &V5, &o) == LPF_OK);
        CHECK(fake_hip_launches() - l0 == 3 * 3);                          // ranges {0}, {1}, {2, 3}
        CHECK(fake_hip_copies() - c0 == 1 + 3 * (3 + 7));
        lpf_match2d_input ind = b.input(1);                               // all on the device: the scratch still bounds a range
        ind.front = nullptr;                                              // (a device front of 20 000 columns would be refused: see refusals)
        lpf_assign2d_outputs od = out.outputs(1);
        CHECK(lpf_assign_2d(c, b.F(), &ind, &V5, &od) == LPF_ERR_ARG);     // front is required with boxes
        Batch d({1024, 1024, 1024, 2}, {1024, 1000, 1024, 5}, false);
        Out dout(d, EVERYTHING);
        lpf_match2d_input din = d.input(1);
        lpf_assign2d_outputs dod = dout.outputs(1);
        const long long l2 = fake_hip_launches(), c2 = fake_hip_copies();
        CHECK(lpf_assign_2d(c, d.F(), &din, &V5, &dod) == LPF_OK);
        CHECK(fake_hip_launches() - l2 == 3 && fake_hip_copies() - c2 == 1);      // one range; only the table is copied
        int64_t st[8];
        CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK);
        CHECK(lpf_assign_2d(c, d.F(), &din, &V5, &dod) == LPF_OK);
        CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK && st[0] == 0 && st[6] == 0 && st[2] == 1);      // no host wait, one ring upload
        Batch e({1024, 1024, 1024, 2}, {1024, 1000, 1024, 5});
        Out eout(e, COL | STATUS);
        lpf_assign_input ein = e.costs(1);
        lpf_assign_outputs eod = eout.costs(1);
        CHECK(lpf_assign_costs(c, e.F(), &ein, &eod) == LPF_OK);
        CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK);
        CHECK(lpf_assign_costs(c, e.F(), &ein, &eod) == LPF_OK);
        CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK && st[0] == 0 && st[6] == 0 && st[2] == 1);
    }
}

int main()
{
    lpf_ctx *c = drive_begin();
    refusals(c);
    runs(c);
    lpf_destroy(c);
    return drive_finish("drive_assign", true);
}
