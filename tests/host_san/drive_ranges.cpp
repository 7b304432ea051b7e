// drive_ranges.cpp -- drives the HOST side of the nine batched analysis calls (lpf_api.hip compiled --offload-host-only with -DLPF_LAB
// against fake_hip.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer with TINY ranges: lpf_lab_set_range_limits cuts a batch of
// six frames (six images for lpf_depth_overlays) into ranges of one and of two items and by a staging budget of one byte, so that
// the staging spans of every call -- the copies up and back of each range -- run over real heap bounds many times instead of twice.
// Checked: the return codes, lpf_lab_last_ranges, and the launches of every range.  Kernel launches do nothing here (fake_hip.cpp):
// the values are checked on the GPU by tests/test_gpu_batch_ranges.py.
#include "drive_common.h"

static const int F = 6;
static const int DETS[F] = {2, 0, 3, 1, 0, 2}, BOXES[F] = {3, 1, 0, 2, 0, 4}, POINTS[F] = {3, 0, 5, 2, 0, 4};   // no detections | no boxes | empty
static const int W = 8, H = 6, M = 2;

template <typename T> static std::vector<T> offsets(const int *n, int count)
{
    std::vector<T> off(1, 0);
    for (int i = 0; i < count; ++i) off.push_back(off.back() + n[i]);
    return off;
}

// the ranges a setting cuts `items` items into, when every item costs more than a byte and a budget cuts the call at all
struct Setting { long long budget; int max_items; };
static const Setting SETTINGS[] = {{0, 1}, {0, 2}, {1, 0}, {1, 1}, {0, 0}};
static std::vector<int> ranges_of(const Setting &s, int items, bool budget_cuts)
{
    int per = items;
    if (s.max_items > 0) per = s.max_items;
    if (s.budget == 1 && budget_cuts) per = 1;
    std::vector<int> first;
    for (int i = 0; i < items; i += per) first.push_back(i);
    first.push_back(items);
    return first;
}

// one call under every setting: launches(first, count) of a range; budget_cuts: plan_ranges plans the call (not a plain frame loop)
template <typename Call, typename Launches> static void sweep(const char *what, int items, bool budget_cuts, Call &&call, Launches &&launches)
{
    const int failed = g_fail;
    for (const Setting &s : SETTINGS) {
        CHECK(lpf_lab_set_range_limits(g_ctx, s.budget, s.max_items) == LPF_OK);
        const std::vector<int> r = ranges_of(s, items, budget_cuts);
        long long want = 0;
        for (size_t k = 0; k + 1 < r.size(); ++k) want += launches(r[k], r[k + 1] - r[k]);
        const long long l0 = fake_hip_launches();
        CHECK(call() == LPF_OK);
        CHECK(lpf_lab_last_ranges(g_ctx) == (int)r.size() - 1);
        CHECK(fake_hip_launches() - l0 == want);
        if (fake_hip_launches() - l0 != want)
            fprintf(stderr, "  %s under budget %lld, max_items %d: %lld launches, expected %lld\n", what, s.budget, s.max_items, fake_hip_launches() - l0, want);
    }
    CHECK(lpf_lab_set_range_limits(g_ctx, 0, 0) == LPF_OK);
    if (g_fail != failed) fprintf(stderr, "  (the failed checks above: %s)\n", what);
}

static int most(const int *n, int first, int count)
{
    int m = 0;
    for (int i = first; i < first + count; ++i) m = n[i] > m ? n[i] : m;
    return m;
}

static void pairs(lpf_ctx *c)
{
    const std::vector<int32_t> det_off = offsets<int32_t>(DETS, F), box_off = offsets<int32_t>(BOXES, F);
    const size_t D = (size_t)det_off[F], B = (size_t)box_off[F];
    size_t P = 0;
    for (int f = 0; f < F; ++f) P += (size_t)DETS[f] * BOXES[f];
    std::vector<float> dets(D * 4, 1.0f);
    std::vector<double> bbox(B * 4, 2.0), cost(P, 0.5);
    std::vector<int32_t> front(B, 1);
    lpf_match2d_input in;
    memset(&in, 0, sizeof in);
    in.dets = dets.data(); in.det_off = det_off.data(); in.bbox2d = bbox.data(); in.front = front.data(); in.box_off = box_off.data();
    in.min_iou = 0.25; in.w_iou = 0.5; in.w_center = 0.3; in.w_size = 0.2;
    std::vector<int32_t> best(D, 7), col(D, 7), status(F, 7), accepted(D, 7);
    std::vector<double> best_iou(D, 7.0), out_cost(P, 7.0), iou(D, 7.0), total(D, 7.0);
    {
        lpf_match2d_outputs o;
        memset(&o, 0, sizeof o);
        o.best_box = best.data(); o.best_iou = best_iou.data(); o.cost = out_cost.data();
        // a range without detections launches nothing
        sweep("lpf_match_2d", F, true, [&] { return lpf_match_2d(c, F, &in, &o); }, [&](int f, int n) { return most(DETS, f, n) > 0 ? 1 : 0; });
    }
    {
        lpf_assign_input ai;
        memset(&ai, 0, sizeof ai);
        ai.cost = cost.data(); ai.det_off = det_off.data(); ai.box_off = box_off.data(); ai.front = front.data();
        lpf_assign_outputs o;
        memset(&o, 0, sizeof o);
        o.col_of_row = col.data(); o.status = status.data();
        sweep("lpf_assign_costs", F, true, [&] { return lpf_assign_costs(c, F, &ai, &o); }, [](int, int) { return 2; });     // pack, solve
    }
    {
        lpf_assign2d_params p = {0.3, 0.15};
        lpf_assign2d_outputs o;
        memset(&o, 0, sizeof o);
        o.box_of_det = col.data(); o.iou = iou.data(); o.total_score = total.data(); o.accepted = accepted.data(); o.status = status.data();
        sweep("lpf_assign_2d", F, true, [&] { return lpf_assign_2d(c, F, &in, &p, &o); }, [](int, int) { return 3; });       // pack, solve, finish
    }
}

static void points(lpf_ctx *c)
{
    const std::vector<int64_t> frame_off = offsets<int64_t>(POINTS, F);
    const std::vector<int32_t> box_off = offsets<int32_t>(BOXES, F);
    const size_t N = (size_t)frame_off[F], B = (size_t)box_off[F];
    std::vector<float> pts(N * 4, 1.0f);
    std::vector<double> corners(B * 24, 1.0);
    CHECK(lpf_set_boxes(c, corners.data(), box_off.data(), F, 1) == LPF_OK);
    {
        const int64_t cap = 4;
        std::vector<int64_t> inst_idx((size_t)F * cap, 0), inst_off((size_t)F * (M + 1), 0), best_cnt((size_t)F * M, 0);
        std::vector<int32_t> best_box((size_t)F * M, -1);
        for (int f = 0; f < F; ++f)                                      // car 0 lists the frame's first points (up to two), car 1 nothing
            for (int m = 0; m < M; ++m) inst_off[(size_t)f * (M + 1) + m + 1] = POINTS[f] < 2 ? POINTS[f] : 2;
        for (int f = 0; f < F; ++f) inst_idx[(size_t)f * cap + 1] = 1;
        lpf_inside_input in;
        memset(&in, 0, sizeof in);
        in.inst_idx = inst_idx.data(); in.inst_cap = cap; in.inst_off = inst_off.data(); in.best_box = best_box.data(); in.best_cnt = best_cnt.data();
        in.M = M; in.min_points = 1;
        std::vector<uint8_t> inside((size_t)F * cap, 7);
        std::vector<int64_t> part_idx((size_t)F * cap, 7), n_inside((size_t)F * M, 7);
        std::vector<float> part_xyz((size_t)F * cap * 3, 7.0f);
        std::vector<int32_t> matched((size_t)F * M, 7);
        lpf_inside_outputs o;
        memset(&o, 0, sizeof o);
        o.inside = inside.data(); o.part_idx = part_idx.data(); o.part_xyz = part_xyz.data(); o.n_inside = n_inside.data(); o.matched = matched.data();
        CHECK(lpf_inside_masks(c, pts.data(), frame_off.data(), F, 0, &in, &o) == LPF_OK);       // (the first call also launches the box tables' preparation)
        sweep("lpf_inside_masks", F, false, [&] { return lpf_inside_masks(c, pts.data(), frame_off.data(), F, 0, &in, &o); }, [](int, int) { return 1; });
    }
    {
        std::vector<int64_t> valid_idx(N ? N : 1, 0), n_valid(F, 0);
        for (int f = 0; f < F; ++f) {
            n_valid[f] = POINTS[f];
            for (int i = 0; i < POINTS[f]; ++i) valid_idx[(size_t)frame_off[f] + i] = i;
        }
        std::vector<uint32_t> labels(N ? N : 1, 1u);
        lpf_box_points_input in;
        memset(&in, 0, sizeof in);
        in.valid_idx = valid_idx.data(); in.n_valid = n_valid.data(); in.label_valid_words = labels.data(); in.LW = 1;
        std::vector<int32_t> box_points(B, 7), box_labelled(B, 7), first_box(N, 7);
        std::vector<int64_t> counts((size_t)F * 4, 7);
        lpf_box_points_outputs o;
        memset(&o, 0, sizeof o);
        o.box_points = box_points.data(); o.box_labelled = box_labelled.data(); o.first_box = first_box.data(); o.frame_counts = counts.data();
        sweep("lpf_box_points", F, false, [&] { return lpf_box_points(c, pts.data(), frame_off.data(), F, 0, &in, &o); }, [](int, int) { return 1; });
    }
    {
        const int mh = 3, mw = 5;
        std::vector<uint8_t> masks((size_t)F * M * mh * mw, 1);
        std::vector<double> colors((size_t)F * M * 3, 0.5);
        lpf_first_match_input in;
        memset(&in, 0, sizeof in);
        in.masks = masks.data(); in.colors = colors.data(); in.M = M; in.mh = mh; in.mw = mw;
        std::vector<int32_t> first_mask(N, 7), car_mask(N, 7);
        std::vector<int64_t> car_idx(N, 7), n_car(F, 7), n_bg(F, 7), mask_count((size_t)F * M, 7);
        std::vector<double> car_rgb(N * 3, 7.0);
        lpf_first_match_outputs o;
        memset(&o, 0, sizeof o);
        o.first_mask = first_mask.data(); o.car_idx = car_idx.data(); o.car_mask = car_mask.data(); o.car_rgb = car_rgb.data();
        o.n_car = n_car.data(); o.n_bg = n_bg.data(); o.mask_count = mask_count.data();
        // count, scan and scatter; a range without points only scans
        sweep("lpf_first_match", F, true, [&] { return lpf_first_match(c, pts.data(), frame_off.data(), F, 0, &in, &o); },
              [&](int f, int n) { return most(POINTS, f, n) > 0 ? 3 : 1; });
    }
    {
        std::vector<uint8_t> masks((size_t)F * M * H * W, 1);
        lpf_wide_input in;
        memset(&in, 0, sizeof in);
        in.masks = masks.data(); in.M = M;
        const int64_t cap = 16;
        std::vector<int64_t> pix((size_t)F * cap, 7), pidx((size_t)F * cap, 7), car_off((size_t)F * (M + 1), 7), need(F, 7);
        std::vector<double> depth((size_t)F * cap, 7.0);
        std::vector<int32_t> overflow(F, 7);
        lpf_depth_maps_outputs o;
        memset(&o, 0, sizeof o);
        o.pix = pix.data(); o.depth = depth.data(); o.point_idx = pidx.data(); o.cap = cap; o.car_off = car_off.data(); o.need = need.data();
        o.overflow = overflow.data();
        // winner, count raster, scan, frame, writing raster; a chunk without points only scans and closes its frames
        sweep("lpf_depth_maps", F, true, [&] { return lpf_depth_maps(c, pts.data(), frame_off.data(), F, 0, &in, &o); },
              [&](int f, int n) { return most(POINTS, f, n) > 0 ? 5 : 2; });
    }
}

static void views_and_overlays(lpf_ctx *c)
{
    {
        const std::vector<int32_t> box_off = offsets<int32_t>(BOXES, F);
        const size_t B = (size_t)box_off[F];
        std::vector<double> corners(B * 24, 1.0), velo(B * 24, 7.0);
        lpf_box_views_input in;
        memset(&in, 0, sizeof in);
        in.corners_cam0 = corners.data(); in.box_off = box_off.data(); in.T_cam_to_velo = IDENT;
        in.min_points_in_view = 4; in.depth_lo = 0.1; in.depth_hi = 100.0; in.min_area = 100.0;
        std::vector<uint8_t> keep(B, 7);
        std::vector<int32_t> kept_pos(B, 7), counts((size_t)F * 6, 7);
        lpf_box_views_outputs o;
        memset(&o, 0, sizeof o);
        o.keep = keep.data(); o.kept_pos = kept_pos.data(); o.frame_counts = counts.data(); o.corners_velo = velo.data();
        sweep("lpf_box_views", F, true, [&] { return lpf_box_views(c, F, &in, &o); }, [](int, int) { return 1; });            // (the counts are always written)
    }
    {
        const int FR = 3;                                                 // 3 frames x 2 cars: six images, ranges of two are whole frames,
        const int64_t cap = 4;                                            // ranges of one cut every frame
        std::vector<int64_t> pix((size_t)FR * cap, 0), car_off((size_t)FR * (M + 1), 0);
        std::vector<double> depth((size_t)FR * cap, 1.0);
        for (int f = 0; f < FR; ++f) {
            int64_t *off = &car_off[(size_t)f * (M + 1)];
            off[1] = f; off[2] = f + 1;                                   // car 0: f pixels, car 1: one
            for (int64_t e = 0; e < off[2]; ++e) pix[(size_t)f * cap + e] = (e < off[1] ? e : 0) + (e >= off[1] ? 5 : 0);
        }
        std::vector<uint8_t> seg((size_t)FR * H * W * 3, 9), images((size_t)FR * M * H * W * 3, 7);
        std::vector<double> mx((size_t)FR * M, 7.0);
        lpf_depth_overlay_input in;
        memset(&in, 0, sizeof in);
        in.pix = pix.data(); in.depth = depth.data(); in.cap = cap; in.car_off = car_off.data(); in.M = M; in.seg = seg.data();
        lpf_depth_overlay_outputs o;
        memset(&o, 0, sizeof o);
        o.images = images.data(); o.max_depth = mx.data();
        sweep("lpf_depth_overlays", FR * M, true, [&] { return lpf_depth_overlays(c, FR, &in, &o); }, [](int, int) { return 2; });     // render, paint
    }
}

int main()
{
    lpf_ctx *c = drive_begin();
    CHECK(lpf_lab_set_range_limits(nullptr, 0, 0) == LPF_ERR_ARG && lpf_lab_last_ranges(nullptr) == LPF_ERR_ARG);
    CHECK(lpf_lab_set_range_limits(c, -1, 0) == LPF_ERR_ARG && lpf_lab_set_range_limits(c, 0, -1) == LPF_ERR_ARG);
    CHECK(lpf_lab_last_ranges(c) == 0);
    const double K[9] = {4.0, 0, 4.0, 0, 4.0, 3.0, 0, 0, 1};
    CHECK(lpf_set_camera(c, IDENT, K, W, H, 0.0, 50.0) == LPF_OK);
    pairs(c);
    points(c);
    views_and_overlays(c);
    lpf_destroy(c);
    return drive_finish("drive_ranges", false);
}
