// drive.cpp -- drives the HOST side of liblpf (lpf_api.hip compiled --offload-host-only against fake_hip.cpp) under a sanitizer:
// argument validation, host-memory runs, the multi-camera, wide and depth-map entry points (host and device outputs, one and several
// frames, their refused arguments and messages), the geometry tables' cache key, the software-pipelined modes with new masks /
// rectangles / boxes / batch shapes every run (the pinned upload ring is lapped several times: > 40 000 small uploads and sizes that
// fill a quarter exactly), the box-set and scratch-set rotation, the graph state machine, mask resize / erosion staging and the
// reader's worker threads; then every source a run's tiles can take their label bits from (mask_sources, mask_transitions) and every
// mask rule / label width of the multi-camera, wide and depth-map packs (pack_forms).  Kernel launches do nothing (fake_hip.cpp), so
// results are not checked here -- the GPU tests do that; what is checked is that every call returns what it should and that the
// sanitizer stays silent.  Which kernels are launched, with which grids, is recorded by fake_hip.cpp: count and hash are printed after
// each section, and FAKE_HIP_TRACE=<file> keeps the lines -- two versions of the host code can be compared launch by launch.
#include "drive_common.h"
#include <algorithm>
#include <string>

static const int W = 128, H = 48;                             // (a small image; pipelined_streams also runs a 1408 x 376 one)

static void fill_outputs(Dev &D, lpf_outputs &o, int64_t n, int F, int M, int Btot, int64_t cap, int on_device)
{
    memset(&o, 0, sizeof o);
    o.uv = D.get<int32_t>(2 * n); o.label_bits = D.get<uint32_t>(n); o.valid_idx = D.get<int64_t>(n);
    o.inst_idx = D.get<int64_t>((size_t)F * cap); o.inst_cap = cap; o.count_mb = D.get<int32_t>((size_t)(M ? M : 1) * (Btot ? Btot : 1));
    o.summary = D.get<lpf_frame_summary>(F); o.uv_valid = D.get<int32_t>(2 * n); o.label_valid = D.get<uint32_t>(n);
    o.on_device = on_device;
}

static void argument_errors()
{
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(nullptr, 0) == LPF_ERR_ARG);
    CHECK(lpf_create(&c, 5) == LPF_ERR_ARG && c == nullptr);
    CHECK(lpf_create(&c, 0) == LPF_OK && c);
    g_ctx = c;
    lpf_outputs o; memset(&o, 0, sizeof o);
    float p4[4] = {1, 2, 3, 0};
    CHECK(lpf_run(c, p4, 1, 0, &o) == LPF_ERR_STATE);                       // no camera yet
    CHECK(lpf_set_masks_u8(c, nullptr, 1, 1, 0, 0) == LPF_ERR_STATE);
    CHECK(lpf_set_camera(c, nullptr, K9, W, H, 0, 50) == LPF_ERR_ARG);
    CHECK(lpf_set_camera(c, T16, K9, 0, H, 0, 50) == LPF_ERR_ARG);
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    CHECK(lpf_set_masks_u8(c, nullptr, 1, 33, 0, 0) == LPF_ERR_ARG);
    CHECK(lpf_set_masks_u8(c, nullptr, 1, 2, 0, 0) == LPF_ERR_ARG);
    CHECK(lpf_set_masks_f32(c, nullptr, 0, 0, 7, 0, 0) == LPF_ERR_ARG);
    CHECK(lpf_set_pipelined(c, 1) == LPF_ERR_ARG && lpf_set_pipelined(c, 3) == LPF_ERR_ARG && lpf_set_pipelined(c, 9) == LPF_ERR_ARG);
    int32_t bad_off[2] = {1, 3};
    double corners[24 * 3] = {0};
    CHECK(lpf_set_boxes(c, corners, bad_off, 1, 1) == LPF_ERR_ARG);
    int32_t desc[3] = {0, 2, 1};
    CHECK(lpf_set_boxes(c, corners, desc, 2, 1) == LPF_ERR_ARG);
    CHECK(lpf_run(c, nullptr, 5, 0, &o) == LPF_ERR_ARG);
    CHECK(lpf_run(c, p4, -1, 0, &o) == LPF_ERR_ARG);
    o.inst_idx = (int64_t *)p4; o.inst_cap = 0;
    CHECK(lpf_run(c, p4, 1, 0, &o) == LPF_ERR_ARG);
    memset(&o, 0, sizeof o);
    o.uv_valid = (int32_t *)p4;
    CHECK(lpf_run(c, p4, 1, 0, &o) == LPF_ERR_ARG);                         // uv_valid needs valid_idx
    CHECK(lpf_graph_end(c, nullptr) == LPF_ERR_ARG);
    lpf_graph *g = nullptr;
    CHECK(lpf_graph_end(c, &g) == LPF_ERR_STATE);
    CHECK(lpf_run_frame(c, nullptr) == LPF_ERR_ARG);
    CHECK(lpf_allreduce_metrics(c, nullptr, 1, 0, nullptr) == LPF_ERR_ARG);
    CHECK(lpf_resize_masks_u8(c, nullptr, 1, 4, 4, nullptr, 0) == LPF_ERR_ARG);
    uint8_t px[64] = {0};
    {
        std::vector<uint8_t> big((size_t)4 * W * H, 1), out((size_t)W * H);
        CHECK(lpf_resize_masks_u8(c, big.data(), 1, 2 * H, 2 * W, out.data(), 0) == LPF_OK);   // the INTER_AREA case: no weight tables
        CHECK(lpf_resize_masks_u8(c, big.data(), 1, 2 * H, W, out.data(), 0) == LPF_OK);       // twice in one axis: linear, with tables
    }
    CHECK(lpf_erode_masks_u8(c, px, 1, 8, 8, 1, px, 0) == LPF_ERR_ARG);          // src == dst
    CHECK(strlen(lpf_build_id()) > 0 && lpf_abi_version() == LPF_ABI_VERSION);
    void *pin = lpf_host_alloc(1000);
    CHECK(pin != nullptr);
    memset(pin, 1, 1000);
    lpf_host_free(pin);
    lpf_destroy(c);
    lpf_destroy(nullptr);
    g_ctx = nullptr;
}

static void host_memory_runs()
{
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(&c, 0) == LPF_OK);
    g_ctx = c;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    Dev D;
    const int F = 3, M = 5;
    const int64_t off[F + 1] = {0, 1000, 1000, 4321};                      // an empty frame in the middle
    std::vector<float> pts(4 * off[F], 1.0f);
    std::vector<uint8_t> masks((size_t)F * M * W * H, 1);
    std::vector<float> fmasks((size_t)F * M * W * H, 1.0f);
    std::vector<double> corners(24 * 7, 0.5);
    const int32_t boff[F + 1] = {0, 3, 3, 7};
    lpf_outputs o;
    fill_outputs(D, o, off[F], F, M, 7, 5000, 0);
    for (int it = 0; it < 3; ++it) {
        CHECK(lpf_set_masks_u8(c, masks.data(), F, M, it, 0) == LPF_OK);
        CHECK(lpf_set_boxes(c, corners.data(), boff, F, it & 1) == LPF_OK);
        CHECK(lpf_run_batch(c, pts.data(), off, F, 0, &o) == LPF_OK);
        CHECK(lpf_set_masks_f32(c, fmasks.data(), F, M, it % 3, it, 0) == LPF_OK);
        CHECK(lpf_run_batch(c, pts.data(), off, F, 0, &o) == LPF_OK);
    }
    std::vector<uint32_t> img((size_t)F * W * H);
    CHECK(lpf_get_label_image(c, img.data(), 0) == LPF_OK);
    CHECK(lpf_set_label_image(c, img.data(), F, M, 0) == LPF_OK);
    CHECK(lpf_run_batch(c, pts.data(), off, F, 0, &o) == LPF_OK);
    CHECK(lpf_run_batch(c, pts.data(), off, 2, 0, &o) == LPF_ERR_STATE);    // masks were set for 3 frames
    // box preparation, stand-alone operators
    std::vector<uint8_t> vis(7), inside(7 * 100);
    std::vector<double> cv(24 * 7), bb(4 * 7);
    std::vector<int32_t> fr(7);
    double Tcv[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    CHECK(lpf_prepare_boxes(c, corners.data(), 7, Tcv, vis.data(), cv.data(), bb.data(), fr.data()) == LPF_OK);
    CHECK(lpf_set_boxes_cam0(c, corners.data(), 0, boff, F, Tcv, 1, 1, vis.data(), cv.data(), bb.data(), fr.data()) == LPF_OK);
    CHECK(lpf_points_in_boxes(c, pts.data(), 100, 4, corners.data(), 7, 1, inside.data(), 0) == LPF_OK);
    std::vector<double> dimg((size_t)W * H);
    std::vector<int32_t> win((size_t)W * H);
    CHECK(lpf_depth_image(c, pts.data(), 1000, 0, dimg.data(), win.data()) == LPF_OK);
    // masks of another size: erosion at their own size, then the resize
    std::vector<uint8_t> small((size_t)2 * 20 * 50, 255), er(small.size()), big((size_t)2 * W * H);
    for (int iters = 0; iters < 4; ++iters) CHECK(lpf_erode_masks_u8(c, small.data(), 2, 20, 50, iters, er.data(), 0) == LPF_OK);
    CHECK(lpf_resize_masks_u8(c, er.data(), 2, 20, 50, big.data(), 0) == LPF_OK);
    CHECK(lpf_resize_masks_u8(c, big.data(), 2, H, W, big.data() /* same size: a copy */, 0) == LPF_OK);
    int64_t st[8];
    CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK && st[0] > 0);
    double ms = 0; int64_t nl = 0;
    CHECK(lpf_profile_enable(c, 1) == LPF_OK && lpf_run_batch(c, pts.data(), off, F, 0, &o) == LPF_OK);
    CHECK(lpf_profile_read(c, &ms, &nl, 1) == LPF_OK && nl == 1 && lpf_profile_overhead(c, &ms) == LPF_OK);
    lpf_destroy(c);
    g_ctx = nullptr;
}

// the software-pipelined modes with everything new every run, long enough to lap the 8 MiB pinned ring several times
static void pipelined_streams(int mode, int runs, const int W, const int H)
{
    // (W x H = 128 x 48: the frames are dense -- masks are packed, the pack rides in mode 4; 1408 x 376: launches of sparse frames are
    //  small here -- at most 6 frames hold 1.6 M points sparsely, the large geometry starts above 3.67 M -- and their tiles read all M
    //  mask bytes of a point, gated by the rectangles; the large launches are dense and packed.  Large sparse launches, whose tiles go
    //  through the rectangles' candidate grid, take 14 frames or more: mask_sources)
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(&c, 0) == LPF_OK);
    g_ctx = c;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    CHECK(lpf_set_pipelined(c, mode) == LPF_OK);
    Dev D;
    const int M = 4, FMAX = 6;
    const int64_t NMAX = (W > 1000) ? 6000000 : 40000;        // (the large image: now and then a launch beyond 3.5 Mi points, the large geometry)
    float *pts = D.get<float>(4 * NMAX);
    uint8_t *masks = D.get<uint8_t>((size_t)FMAX * M * W * H);
    double *dcorners = D.get<double>(24 * 64);
    int32_t *drects = D.get<int32_t>((size_t)FMAX * M * 4);
    std::vector<double> hcorners(24 * 11000, 0.25);
    std::vector<int32_t> hrects((size_t)FMAX * M * 4, 3);
    lpf_outputs o;
    fill_outputs(D, o, NMAX, FMAX, M, 11000, NMAX, 1);
    double Tcv[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    unsigned rng = 12345u + (unsigned)mode;
    auto rnd = [&](unsigned n) { rng = rng * 1664525u + 1013904223u; return (rng >> 8) % n; };
    for (int it = 0; it < runs; ++it) {
        const int F = 1 + (int)rnd(FMAX);
        int64_t off[FMAX + 1];
        off[0] = 0;
        const unsigned per_frame = (W > 1000 && it % 7 != 0) ? 200000u : (unsigned)(NMAX / FMAX);     // (mostly sparse frames on the large image)
        for (int f = 0; f < F; ++f) off[f + 1] = off[f] + (int64_t)rnd(per_frame);
        // rectangles from host memory (F * M * 16 bytes <= 384: the 256-byte pieces that walked the ring's head to its end) or lent
        if (it % 3 != 2) CHECK(lpf_set_mask_rects(c, it % 3 ? hrects.data() : drects, it % 3 ? 0 : 1, F, M) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        int32_t boff[FMAX + 1];
        boff[0] = 0;
        // mostly a few boxes; now and then sizes that fill a quarter of the ring exactly (192 B per box: 10922 boxes = 2 MiB - 128 B)
        const int per = (it % 97 == 0) ? 10922 / F : (int)rnd(9);
        for (int f = 0; f < F; ++f) boff[f + 1] = boff[f] + per;
        if (it % 5 == 0) CHECK(lpf_set_boxes_cam0(c, dcorners, 2, boff, F, Tcv, 1, 1, nullptr, nullptr, nullptr, nullptr) == (boff[F] <= 64 ? LPF_OK : LPF_OK));
        else CHECK(lpf_set_boxes_ex(c, hcorners.data(), 0, boff, F, it & 1) == LPF_OK);
        if (boff[F] > 64 && it % 5 == 0) CHECK(lpf_set_boxes_ex(c, hcorners.data(), 0, boff, F, 1) == LPF_OK);   // (the lent array holds 64 boxes)
        if (F == 1 && it % 4 == 0) {                       // the one-call form: rectangles, lent masks, lent cam-0 corners, the run
            lpf_frame_job j;
            memset(&j, 0, sizeof j);
            j.pts = pts; j.n_points = off[1]; j.masks = masks; j.mask_rects = drects; j.n_masks = M;
            j.corners_cam0 = dcorners; j.n_boxes = 17; j.T_cam_to_velo = Tcv; j.filter_visible = 1; j.oriented = 1; j.out = o;
            CHECK(lpf_run_frame(c, &j) == LPF_OK);
        } else {
            CHECK(lpf_run_batch(c, pts, off, F, 1, &o) == LPF_OK);
        }
        if (it % 1000 == 999) CHECK(lpf_release_to_stream(c, nullptr) == LPF_OK);
    }
    int64_t st[8];
    CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK);
    fprintf(stderr, "  mode %d: %d runs, uploads %lld, blocking uploads %lld, host waits %lld, drains %lld, step launches %lld\n", mode, runs,
            (long long)st[2], (long long)st[6], (long long)st[0], (long long)st[1], (long long)st[3]);
    CHECK(st[2] > runs);                                                     // the ring was really used
    CHECK(lpf_sync(c) == LPF_OK);
    CHECK(lpf_set_pipelined(c, 0) == LPF_OK);
    lpf_destroy(c);
    g_ctx = nullptr;
}

static void fill_wide_outputs(Dev &D, lpf_wide_outputs &o, int64_t n, int F, int M, int Btot, int64_t cap, int on_device)
{
    const int LW = M > 0 ? (M + 31) / 32 : 1;
    memset(&o, 0, sizeof o);
    o.uv = D.get<int32_t>(2 * n); o.depth = D.get<double>(n); o.u_f = D.get<double>(n); o.v_f = D.get<double>(n);
    o.valid_idx = D.get<int64_t>(n); o.uv_valid = D.get<int32_t>(2 * n); o.label_words = D.get<uint32_t>(n * LW);
    o.label_valid_words = D.get<uint32_t>(n * LW); o.inst_idx = D.get<int64_t>((size_t)F * cap); o.inst_cap = cap;
    o.count_mb = D.get<int32_t>((size_t)(M ? M : 1) * (Btot ? Btot : 1)); o.n_valid = D.get<int64_t>(F); o.n_labelled = D.get<int64_t>(F);
    o.inst_count = D.get<int64_t>((size_t)F * M + 1); o.inst_off = D.get<int64_t>((size_t)F * (M + 1)); o.best_cnt = D.get<int64_t>((size_t)F * M + 1);
    o.best_box = D.get<int32_t>((size_t)F * M + 1); o.inst_overflow = D.get<int32_t>(F);
    o.on_device = on_device;
}

// lpf_run_cams, lpf_run_cams_wide, lpf_run_wide, lpf_run_frame_wide and lpf_depth_maps: host and device outputs, one and several frames,
// host and device masks (uint8 and float, with and without rectangles and erosion), and one of each refused argument
static void wide_and_multicam_runs()
{
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(&c, 0) == LPF_OK);
    g_ctx = c;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    Dev D;
    const int FMAX = 3, MW = 40;                               // (MW: more masks than a narrow run takes)
    const int64_t offs[2][FMAX + 1] = {{0, 2500, 0, 0}, {0, 1000, 1000, 4321}};     // one frame; three with an empty one in the middle
    const int64_t NMAX = offs[1][FMAX];
    std::vector<float> hpts(4 * NMAX, 1.0f);
    float *dpts = D.get<float>(4 * NMAX);
    const size_t hw = (size_t)W * H;
    std::vector<uint8_t> hmasks((size_t)FMAX * MW * hw, 1);
    uint8_t *dmasks = D.get<uint8_t>((size_t)FMAX * MW * hw);
    std::vector<float> hfmasks((size_t)FMAX * 5 * hw, 1.0f);
    float *dfmasks = D.get<float>((size_t)FMAX * 5 * hw);
    std::vector<int32_t> hrects((size_t)FMAX * MW * 4, 2);
    int32_t *drects = D.get<int32_t>((size_t)FMAX * MW * 4);
    std::vector<double> hcorners(24 * 9, 0.5);
    double *dcorners = D.get<double>(24 * 9);
    const int32_t boffs[2][FMAX + 1] = {{0, 4, 0, 0}, {0, 3, 3, 9}};
    for (int shape = 0; shape < 2; ++shape) {
        const int F = shape ? FMAX : 1;
        const int64_t *off = offs[shape];
        const int32_t *boff = boffs[shape];
        const int64_t n = off[F];
        for (int on_device = 0; on_device < 2; ++on_device) {
            const float *pts = on_device ? dpts : hpts.data();
            // three cameras: uint8 masks with rectangles and host boxes; float masks eroded, with device boxes; no masks, no boxes, 12 px wide
            lpf_cam_input cams[3];
            memset(cams, 0, sizeof cams);
            for (int k = 0; k < 3; ++k) {
                memcpy(cams[k].T_velo_to_rect, T16, sizeof T16);
                memcpy(cams[k].K, K9, sizeof K9);
                cams[k].W = k == 2 ? 12 : W; cams[k].H = H; cams[k].depth_min_excl = 0; cams[k].depth_max_excl = 50;
            }
            cams[0].masks.masks = on_device ? (const void *)dmasks : hmasks.data(); cams[0].masks.rects = on_device ? drects : hrects.data();
            cams[0].masks.M = 5; cams[0].masks.on_device = on_device;
            cams[0].corners_velo = hcorners.data(); cams[0].box_off = boff; cams[0].boxes_on_device = 0; cams[0].oriented = 1;
            cams[1].masks.masks = on_device ? (const void *)dfmasks : hfmasks.data(); cams[1].masks.M = 5; cams[1].masks.f32 = 1;
            cams[1].masks.binarize = 1; cams[1].masks.erode_iters = 2; cams[1].masks.on_device = on_device;
            cams[1].corners_velo = dcorners; cams[1].box_off = boff; cams[1].boxes_on_device = 1 + on_device; cams[1].oriented = 0;
            lpf_outputs o[3];
            for (int k = 0; k < 3; ++k) fill_outputs(D, o[k], n, F, 5, boff[F], 3000, (on_device + k) & 1);   // (host and device outputs in one pass)
            CHECK(lpf_run_cams(c, pts, off, F, on_device, cams, 3, o) == LPF_OK);
            CHECK(lpf_run_cams(c, pts, off, F, on_device, cams, 1, o) == LPF_OK);
            // the same cameras with up to MW masks each
            cams[0].masks.M = MW;
            lpf_wide_outputs ow[3];
            for (int k = 0; k < 3; ++k) fill_wide_outputs(D, ow[k], n, F, cams[k].masks.M, boff[F], 3000, (on_device + k) & 1);
            CHECK(lpf_run_cams_wide(c, pts, off, F, on_device, cams, 3, ow) == LPF_OK);
            // one camera's worth through lpf_run_wide and lpf_depth_maps, with and without the context's boxes
            CHECK(lpf_set_boxes_ex(c, hcorners.data(), 0, boff, F, 1) == LPF_OK);
            for (int k = 0; k < 2; ++k) {
                lpf_wide_outputs w1;
                fill_wide_outputs(D, w1, n, F, cams[k].masks.M, boff[F], 3000, on_device);
                CHECK(lpf_run_wide(c, pts, off, F, on_device, &cams[k].masks, &w1) == LPF_OK);
                lpf_depth_maps_outputs dm;
                memset(&dm, 0, sizeof dm);
                dm.cap = 500; dm.pix = D.get<int64_t>((size_t)F * 500); dm.depth = D.get<double>((size_t)F * 500);
                dm.point_idx = D.get<int64_t>((size_t)F * 500); dm.car_off = D.get<int64_t>((size_t)F * (cams[k].masks.M + 1));
                dm.need = D.get<int64_t>(F); dm.overflow = D.get<int32_t>(F); dm.on_device = on_device;
                CHECK(lpf_depth_maps(c, pts, off, F, on_device, &cams[k].masks, &dm) == LPF_OK);
                CHECK(lpf_depth_maps(c, pts, off, 0, on_device, &cams[k].masks, &dm) == LPF_OK);      // no frames: nothing to do
            }
            CHECK(lpf_set_boxes_ex(c, nullptr, 0, nullptr, 0, 1) == LPF_OK);
        }
    }
    // lpf_run_frame_wide: masks read directly (sparse frame, aligned rectangles) or packed; with and without boxes
    for (int direct = 0; direct < 2; ++direct) {
        lpf_frame_job_wide j;
        memset(&j, 0, sizeof j);
        j.pts = dpts; j.n_points = direct ? 1000 : 4000; j.masks = dmasks; j.mask_rects = direct ? drects : nullptr; j.n_masks = MW;
        j.corners_cam0 = direct ? dcorners : nullptr; j.n_boxes = 9; j.T_cam_to_velo = T16; j.filter_visible = 1; j.oriented = 1;
        fill_wide_outputs(D, j.out, j.n_points, 1, MW, 9, 3000, 1);
        CHECK(lpf_run_frame_wide(c, &j) == LPF_OK);
    }

    // ---- refused arguments (the messages are part of the interface: the Python layer passes them on) ----------------------------------
    const int64_t bad0[2] = {1, 5}, neg[3] = {0, 7, 3}, huge[2] = {0, 0x7fffffffll};
    lpf_cam_input cam;
    memset(&cam, 0, sizeof cam);
    memcpy(cam.T_velo_to_rect, T16, sizeof T16); memcpy(cam.K, K9, sizeof K9); cam.W = W; cam.H = H; cam.depth_max_excl = 50;
    lpf_outputs on;
    fill_outputs(D, on, 1000, 1, 5, 1, 100, 1);
    lpf_wide_outputs owd;
    fill_wide_outputs(D, owd, 1000, 1, 5, 1, 100, 1);
    const int64_t off1[2] = {0, 1000};
    CHECK(lpf_run_cams(c, dpts, off1, 1, 1, &cam, 0, &on) == LPF_ERR_ARG && err_is("run_cams: C=0 cameras, a pass takes 1 .. LPF_MAX_CAMS = 4"));
    CHECK(lpf_run_cams(c, dpts, bad0, 1, 1, &cam, 1, &on) == LPF_ERR_ARG && err_is("run_cams: frame_off[0] must be 0"));
    CHECK(lpf_run_cams_wide(c, dpts, neg, 2, 1, &cam, 1, &owd) == LPF_ERR_ARG && err_is("run_cams_wide: frame 1 has -4 points"));
    CHECK(lpf_run_cams(c, nullptr, off1, 1, 1, &cam, 1, &on) == LPF_ERR_ARG && err_is("run_cams: pts is NULL"));
    cam.W = 0;
    CHECK(lpf_run_cams(c, dpts, off1, 1, 1, &cam, 1, &on) == LPF_ERR_ARG && err_is("run_cams: camera 0 is 0 x 48"));
    cam.W = W; cam.masks.M = 33;
    CHECK(lpf_run_cams(c, dpts, off1, 1, 1, &cam, 1, &on) == LPF_ERR_ARG &&
          err_is("run_cams: camera 0 has M=33 masks per frame, a pass takes 0 .. LPF_MAX_MASKS = 32 per camera (more: lpf_run_wide for that camera)"));
    cam.masks.M = 257;
    CHECK(lpf_run_cams_wide(c, dpts, off1, 1, 1, &cam, 1, &owd) == LPF_ERR_ARG &&
          err_is("run_cams_wide: camera 0 has M=257 masks per frame, a pass takes 0 .. LPF_MAX_MASKS_WIDE = 256 per camera"));
    cam.masks.M = 2;
    CHECK(lpf_run_cams(c, dpts, off1, 1, 1, &cam, 1, &on) == LPF_ERR_ARG &&
          err_is("run_cams: camera 0: erode_iters=0 f32=0 binarize=0 masks=(nil)"));
    cam.masks.masks = dmasks; cam.masks.f32 = 1; cam.masks.binarize = 3;
    CHECK(lpf_run_cams_wide(c, dpts, off1, 1, 1, &cam, 1, &owd) == LPF_ERR_ARG);
    cam.masks.f32 = 0; cam.masks.binarize = 0;
    cam.corners_velo = dcorners; cam.box_off = boffs[1] + 1;                    // (starts at 3)
    CHECK(lpf_run_cams(c, dpts, off1, 1, 1, &cam, 1, &on) == LPF_ERR_ARG && err_is("run_cams: camera 0: box_off must be given and start at 0"));
    const int32_t desc[3] = {0, 5, 2};
    cam.box_off = desc;
    CHECK(lpf_run_cams(c, dpts, neg, 2, 1, &cam, 1, &on) == LPF_ERR_ARG);      // (the frames are checked first)
    const int64_t off2[3] = {0, 500, 1000};
    CHECK(lpf_run_cams(c, dpts, off2, 2, 1, &cam, 1, &on) == LPF_ERR_ARG && err_is("run_cams: camera 0: box_off not ascending at 1"));
    cam.box_off = boffs[0]; cam.boxes_on_device = 3;
    CHECK(lpf_run_cams_wide(c, dpts, off1, 1, 1, &cam, 1, &owd) == LPF_ERR_ARG && err_is("run_cams_wide: camera 0: boxes_on_device=3"));
    cam.boxes_on_device = 0;
    on.inst_cap = 0;
    CHECK(lpf_run_cams(c, dpts, off1, 1, 1, &cam, 1, &on) == LPF_ERR_ARG && err_is("run_cams: out[0].inst_idx given with inst_cap=0"));
    on.inst_cap = 100; on.valid_idx = nullptr;
    CHECK(lpf_run_cams(c, dpts, off1, 1, 1, &cam, 1, &on) == LPF_ERR_ARG);
    owd.inst_cap = 0;
    CHECK(lpf_run_cams_wide(c, dpts, off1, 1, 1, &cam, 1, &owd) == LPF_ERR_ARG && err_is("run_cams_wide: out[0].inst_idx given with inst_cap=0"));
    CHECK(lpf_run_wide(c, dpts, off1, 1, 1, &cam.masks, &owd) == LPF_ERR_ARG && err_is("run_wide: inst_idx given with inst_cap=0"));
    owd.inst_cap = 100;
    CHECK(lpf_run_wide(c, dpts, off1, 1, 1, nullptr, &owd) == LPF_ERR_ARG);
    lpf_wide_input wi = cam.masks;
    wi.M = 300;
    CHECK(lpf_run_wide(c, dpts, off1, 1, 1, &wi, &owd) == LPF_ERR_ARG &&
          err_is("run_wide: M=300 masks per frame, lpf_run_wide takes 0 .. LPF_MAX_MASKS_WIDE = 256"));
    wi.M = 2; wi.erode_iters = -1;
    CHECK(lpf_run_wide(c, dpts, off1, 1, 1, &wi, &owd) == LPF_ERR_ARG && strncmp(lpf_last_error(c), "run_wide: erode_iters=-1 f32=0 binarize=0 masks=", 48) == 0);
    wi.erode_iters = 0;
    CHECK(lpf_run_wide(c, dpts, bad0, 1, 1, &wi, &owd) == LPF_ERR_ARG && err_is("run_wide: frame_off[0] must be 0"));
    CHECK(lpf_run_wide(c, dpts, huge, 1, 1, &wi, &owd) == LPF_ERR_ARG && err_is("run_wide: frame 0 has 2147483647 points"));
    CHECK(lpf_run_wide(c, nullptr, off1, 1, 1, &wi, &owd) == LPF_ERR_ARG && err_is("run_wide: pts is NULL"));
    lpf_depth_maps_outputs dm;
    memset(&dm, 0, sizeof dm);
    dm.car_off = D.get<int64_t>(8); dm.need = D.get<int64_t>(2); dm.on_device = 1;
    wi.M = 300;
    CHECK(lpf_depth_maps(c, dpts, off1, 1, 1, &wi, &dm) == LPF_ERR_ARG &&
          err_is("depth_maps: M=300 masks per frame, lpf_depth_maps takes 0 .. LPF_MAX_MASKS_WIDE = 256"));
    wi.M = 2; wi.f32 = 1; wi.binarize = -1;
    CHECK(lpf_depth_maps(c, dpts, off1, 1, 1, &wi, &dm) == LPF_ERR_ARG && strncmp(lpf_last_error(c), "depth_maps: erode_iters=0 f32=1 binarize=-1", 43) == 0);
    wi.f32 = 0; wi.binarize = 0;
    CHECK(lpf_depth_maps(c, dpts, bad0, 1, 1, &wi, &dm) == LPF_ERR_ARG && err_is("depth_maps: frame_off[0] must be 0"));
    CHECK(lpf_depth_maps(c, dpts, neg, 2, 1, &wi, &dm) == LPF_ERR_ARG && err_is("depth_maps: frame 1 has -4 points"));
    CHECK(lpf_depth_maps(c, nullptr, off1, 1, 1, &wi, &dm) == LPF_ERR_ARG && err_is("depth_maps: pts is NULL"));
    dm.car_off = nullptr;
    CHECK(lpf_depth_maps(c, dpts, off1, 1, 1, &wi, &dm) == LPF_ERR_ARG);
    lpf_frame_job_wide j;
    memset(&j, 0, sizeof j);
    j.pts = dpts; j.n_points = 10; j.n_masks = 300; j.out = owd;
    CHECK(lpf_run_frame_wide(c, nullptr) == LPF_ERR_ARG);
    CHECK(lpf_run_frame_wide(c, &j) == LPF_ERR_ARG);
    j.n_masks = 3;
    CHECK(lpf_run_frame_wide(c, &j) == LPF_ERR_ARG);                            // masks NULL
    j.out.on_device = 0;
    CHECK(lpf_run_frame_wide(c, &j) == LPF_ERR_ARG);
    // every entry point but lpf_run_batch refuses a graph capture
    CHECK(lpf_graph_begin(c) == LPF_OK);
    CHECK(lpf_run_cams(c, dpts, off1, 1, 1, &cam, 1, &on) == LPF_ERR_STATE &&
          err_is("lpf_run_cams cannot be captured into a graph (call it outside lpf_graph_begin ... lpf_graph_end) [the graph capture in progress was abandoned]"));
    lpf_destroy(c);
    g_ctx = nullptr;
}

// The geometry tables of a scratch set are keyed by the frame records AND the count blocks' parts: a fused run of a frame or two (count
// blocks in four parts) and an in-order host-output run of the same shape and box counts (one part) share scratch set 0 -- the first
// run after lpf_set_pipelined uses it, a host-output run always does -- and the second of them must upload its own tables.
static void table_key()
{
    Dev D;
    const int F = 3, M = 2;
    const int64_t off[F + 1] = {0, 1000, 1000, 3000};
    const int32_t boff[F + 1] = {0, 2, 2, 70};                   // (two 64-box words in frame 2)
    float *dpts = D.get<float>(4 * off[F]);
    std::vector<float> hpts(4 * off[F], 1.0f);
    uint8_t *dmasks = D.get<uint8_t>((size_t)F * M * W * H);
    std::vector<double> corners(24 * boff[F], 0.5);
    lpf_outputs od, oh;
    fill_outputs(D, od, off[F], F, M, boff[F], 500, 1);
    fill_outputs(D, oh, off[F], F, M, boff[F], 500, 0);
    for (int fused_first = 1; fused_first >= 0; --fused_first) {
        lpf_ctx *c = nullptr;
        CHECK(lpf_create(&c, 0) == LPF_OK);
        g_ctx = c;
        CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
        CHECK(lpf_set_pipelined(c, 2) == LPF_OK);
        CHECK(lpf_set_boxes_ex(c, corners.data(), 0, boff, F, 1) == LPF_OK);
        for (int r = 0; r < 2; ++r) {
            const bool fused = (r == 0) == (fused_first == 1);
            CHECK(lpf_set_masks_u8(c, dmasks, F, M, 0, 2) == LPF_OK);
            int64_t st[8];
            CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK);
            CHECK(lpf_run_batch(c, fused ? dpts : hpts.data(), off, F, fused ? 1 : 0, fused ? &od : &oh) == LPF_OK);
            CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK);
            CHECK(st[2] == 1);                                   // the run's tables went up through the pinned ring
        }
        CHECK(lpf_sync(c) == LPF_OK);
        lpf_destroy(c);
        g_ctx = nullptr;
    }
}

// the ring alone: 256-byte uploads by the ten thousand (the head reached the end of the buffer after 32768 of them)
static void ring_of_small_uploads()
{
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(&c, 0) == LPF_OK);
    g_ctx = c;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    std::vector<int32_t> rects(4 * 16, 1);
    for (int it = 0; it < 70000; ++it) CHECK(lpf_set_mask_rects(c, rects.data(), 0, 1 + it % 4, 4) == LPF_OK);
    int64_t st[8];
    CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK && st[2] == 70000);
    lpf_destroy(c);
    g_ctx = nullptr;
}

static void graphs()
{
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(&c, 0) == LPF_OK);
    g_ctx = c;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    Dev D;
    const int M = 3;
    const int64_t N = 5000;
    float *pts = D.get<float>(4 * N);
    uint8_t *masks = D.get<uint8_t>((size_t)M * W * H);
    double *corners = D.get<double>(24 * 5);
    const int32_t boff[2] = {0, 5};
    lpf_outputs o;
    fill_outputs(D, o, N, 1, M, 5, N, 1);
    auto frame = [&]() {
        CHECK(lpf_set_masks_u8(c, masks, 1, M, 1, 1) == LPF_OK);
        CHECK(lpf_set_boxes_ex(c, corners, 1, boff, 1, 1) == LPF_OK);
        CHECK(lpf_run(c, pts, N, 1, &o) == LPF_OK);
    };
    frame();                                                                // the shapes once before the capture
    CHECK(lpf_set_pipelined(c, 2) == LPF_OK && lpf_graph_begin(c) == LPF_ERR_STATE && lpf_set_pipelined(c, 0) == LPF_OK);
    CHECK(lpf_graph_begin(c) == LPF_OK && lpf_graph_begin(c) == LPF_ERR_STATE);     // (an error inside a capture abandons it)
    lpf_graph *g0 = nullptr;
    CHECK(lpf_graph_end(c, &g0) == LPF_ERR_STATE);
    CHECK(lpf_graph_begin(c) == LPF_OK);
    frame();
    lpf_graph *g = nullptr;
    CHECK(lpf_graph_end(c, &g) == LPF_OK && g);
    for (int i = 0; i < 5; ++i) CHECK(lpf_graph_launch(c, g) == LPF_OK);
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 30) == LPF_OK);               // anything the graph baked in: stale
    CHECK(lpf_graph_launch(c, g) == LPF_ERR_STATE);
    lpf_graph_destroy(g);
    // an error inside a capture abandons it; the context stays usable
    frame();
    CHECK(lpf_graph_begin(c) == LPF_OK);
    uint8_t host_masks[1] = {0};
    CHECK(lpf_set_masks_u8(c, host_masks, 1, M + 40, 0, 1) == LPF_ERR_ARG);
    CHECK(lpf_graph_end(c, &g) == LPF_ERR_STATE);
    frame();
    CHECK(lpf_graph_begin(c) == LPF_OK);
    std::vector<float> big(4 * 4 * N);
    lpf_outputs ob;
    fill_outputs(D, ob, 4 * N, 1, M, 5, 4 * N, 1);
    float *bigpts = D.get<float>(4 * 4 * N);
    CHECK(lpf_run(c, bigpts, 4 * N, 1, &ob) == LPF_ERR_STATE);              // a buffer would have to grow inside the capture
    frame();
    lpf_graph_destroy(nullptr);
    lpf_destroy(c);
    g_ctx = nullptr;
}

static void reader(const char *tmpdir)
{
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(&c, 0) == LPF_OK);
    g_ctx = c;
    std::vector<std::string> paths;
    for (int i = 0; i < 12; ++i) {
        std::string p = std::string(tmpdir) + "/scan" + std::to_string(i) + ".bin";
        if (i != 4) {                                                       // scan 4 is missing
            FILE *f = fopen(p.c_str(), "wb");
            std::vector<float> v((size_t)4 * (100 + 37 * i) + (i == 7 ? 3 : 0), (float)i);      // scan 7 is not [N][4]
            fwrite(v.data(), 4, v.size(), f);
            fclose(f);
        }
        paths.push_back(p);
    }
    // the frames' box files ride along: scan i has i boxes (file 3 is absent, file 5 has a key the schema lacks, file 6 is cut short)
    std::vector<std::string> bpaths;
    for (int i = 0; i < 12; ++i) {
        std::string p = std::string(tmpdir) + "/BBoxes_" + std::to_string(i) + ".json";
        if (i != 3) {
            std::string t = "[";
            for (int b = 0; b < i; ++b) {
                t += std::string(b ? ",\n " : "") + "{\"index\": " + std::to_string(100 * i + b) + ", \"corners_cam0\": [";
                for (int k = 0; k < 8; ++k) t += std::string(k ? ", " : "") + "[" + std::to_string(i) + ".5, -" + std::to_string(b) + "e-1, " + std::to_string(k) + "]";
                t += i == 5 ? "], \"label\": 1}" : "]}";
            }
            t += "]";
            if (i == 6) t.resize(t.size() / 2);
            FILE *f = fopen(p.c_str(), "wb");
            fwrite(t.data(), 1, t.size(), f);
            fclose(f);
        }
        bpaths.push_back(p);
    }
    lpf_reader *rd = nullptr;
    CHECK(lpf_reader_create(c, &rd, 1, 1000) == LPF_ERR_ARG);
    CHECK(lpf_reader_create(c, &rd, 3, 600) == LPF_OK && rd);
    {
        int nb = -1, st = -1;
        CHECK(lpf_reader_boxes(rd, nullptr, nullptr, &nb, &st) == LPF_ERR_STATE);                // nothing handed out yet
    }
    for (int i = 0; i < 12; ++i) CHECK(lpf_reader_submit_frame(rd, paths[(size_t)i].c_str(), i == 11 ? nullptr : bpaths[(size_t)i].c_str()) == LPF_OK);
    for (int i = 0; i < 12; ++i) {
        const float *d = nullptr, *h = nullptr;
        int64_t n = 0;
        const int rc = lpf_reader_next(rd, &d, &h, &n);
        if (i == 4 || i == 7 || 100 + 37 * i > 600) CHECK(rc == LPF_ERR_IO);
        else { CHECK(rc == LPF_OK && n == 100 + 37 * i && h && d && h[0] == (float)i && d[4 * n - 1] == (float)i); CHECK(lpf_reader_wait(rd) == LPF_OK); }
        const double *bc = nullptr; const int32_t *bi = nullptr;
        int nb = -1, st = -1;
        CHECK(lpf_reader_boxes(rd, &bc, &bi, &nb, &st) == LPF_OK);                                 // (a failed scan still has its box file)
        if (i == 11) CHECK(st == LPF_BOXES_NONE && nb == 0 && !bc);
        else if (i == 3) CHECK(st == LPF_BOXES_ABSENT && nb == 0);
        else if (i == 5 || i == 6) CHECK(st == LPF_BOXES_OTHER && nb == 0 && !bc && !bi);
        else {
            CHECK(st == LPF_BOXES_PARSED && nb == i);
            for (int b = 0; b < nb; ++b)
                CHECK(bi[b] == 100 * i + b && bc[24 * b] == i + 0.5 && bc[24 * b + 1] == -(double)b / 10.0 && bc[24 * b + 23] == 7.0);
        }
    }
    for (int i = 0; i < 3; ++i) CHECK(lpf_reader_submit(rd, paths[i].c_str()) == LPF_OK);      // destroyed with scans still queued
    lpf_reader_destroy(rd);
    lpf_destroy(c);
    g_ctx = nullptr;
}

// lpf_parse_boxes_json on every prefix of a file and on a few thousand damaged copies of it: whatever the bytes, the parser stays inside
// its buffer (ASan) and either parses or says OTHER
static void box_files(const char *tmpdir)
{
    std::string good = "[";
    for (int b = 0; b < 3; ++b) {
        good += std::string(b ? ", " : "") + "{\"index\": " + std::to_string(b - 1) + ", \"corners_cam0\": [";
        for (int k = 0; k < 8; ++k) good += std::string(k ? "," : "") + "[-1.25e1, 2, 0.30000000000000004]";
        good += "]}";
    }
    good += "]\n";
    const std::string p = std::string(tmpdir) + "/BBoxes_fuzz.json";
    auto run = [&](const std::string &text, int &nb, int &st, double *cs, int32_t *ix, int cap) {
        FILE *f = fopen(p.c_str(), "wb");
        fwrite(text.data(), 1, text.size(), f);
        fclose(f);
        return lpf_parse_boxes_json(p.c_str(), cs, ix, cap, &nb, &st);
    };
    double cs[4 * 24]; int32_t ix[4];
    int nb = -1, st = -1;
    CHECK(run(good, nb, st, cs, ix, 4) == LPF_OK && st == LPF_BOXES_PARSED && nb == 3 && ix[0] == -1 && ix[2] == 1 && cs[0] == -12.5 && cs[71] == 0.30000000000000004);
    CHECK(run(good, nb, st, cs, ix, 2) == LPF_ERR_ARG && nb == 3);
    CHECK(run(good, nb, st, nullptr, nullptr, 0) == LPF_ERR_ARG && nb == 3);
    for (size_t k = 0; k + 2 < good.size(); ++k) CHECK(run(good.substr(0, k), nb, st, cs, ix, 4) == LPF_OK && st == LPF_BOXES_OTHER && nb == 0);
    uint32_t x = 12345;
    auto rnd = [&x] { x = x * 1664525u + 1013904223u; return x >> 8; };
    int parsed = 0;
    for (int it = 0; it < 4000; ++it) {
        std::string t = good;
        const int edits = 1 + (int)(rnd() % 3);
        for (int e = 0; e < edits; ++e) {
            const size_t at = rnd() % t.size();
            switch (rnd() % 4) {
            case 0: t[at] = (char)(rnd() & 0xff); break;
            case 1: t.erase(at, 1 + rnd() % 4); break;
            case 2: t.insert(at, 1, "0123456789.eE+-[]{},:\" \n"[rnd() % 24]); break;
            default: t[at] = "0123456789.eE+-[]{},:\" \n"[rnd() % 24]; break;
            }
            if (t.empty()) t = " ";
        }
        const int rc = run(t, nb, st, cs, ix, 4);
        CHECK((rc == LPF_OK && (st == LPF_BOXES_OTHER || (st == LPF_BOXES_PARSED && nb <= 4))) || (rc == LPF_ERR_ARG && nb > 4));
        parsed += st == LPF_BOXES_PARSED;
    }
    CHECK(parsed > 0 && parsed < 4000);                                   // (a changed digit still parses; a lost bracket does not)
    remove(p.c_str());
    CHECK(run("", nb, st, cs, ix, 4) == LPF_OK && st == LPF_BOXES_OTHER);
    remove(p.c_str());
    CHECK(lpf_parse_boxes_json(p.c_str(), cs, ix, 4, &nb, &st) == LPF_OK && st == LPF_BOXES_ABSENT);
}

// ---- where a run's tiles get their label bits -------------------------------------------------------------------------------------
// lpf_run_batch on one context per mode and image size, for every kind of masks (uint8; float under each of the three rules), from host
// memory, device memory that is copied (on_device 1) or lent (2), 16-byte aligned or not, M = 0 / 5 / 12 / 32 (no label image; label
// elements of 1, 2 and 4 bytes), with and without rectangles, with and without erosion -- each in launches of every shape the run tells
// apart: small sparse (the tiles read the masks themselves), small dense in 512- and 1024-point tiles, large dense, and on the large
// image large sparse (14 frames or more: with rectangles the tiles read the masks inside them, through the candidate grid).  Every
// combination runs once with new boxes (the box job rides with the tiles) and once without; every fifth goes through host memory
// (points and outputs), which a pipelined context runs in order after packing what was lent.
static void mask_sources(int mode, const int W, const int H)
{
    const bool big = W > 1000;
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(&c, 0) == LPF_OK);
    g_ctx = c;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    if (mode) CHECK(lpf_set_pipelined(c, mode) == LPF_OK);
    Dev D;
    struct Shape { int F; int64_t n; };
    const Shape small_shapes[4] = {{3, 1700}, {2, 30000}, {1, 1000000}, {2, 4000000}};
    const Shape big_shapes[2] = {{1, 100000}, {16, 3800000}};      // (3.8 M points: beyond LPF_SMALL_LAUNCH, and 2 N <= 16 W H)
    const Shape *shapes = big ? big_shapes : small_shapes;
    const int nshape = big ? 2 : 4, FMAX = big ? 16 : 3;
    const int64_t NMAX = 4000000, NHOST = 30000;
    const size_t hw = (size_t)W * H;
    float *pts = D.get<float>(4 * NMAX);
    std::vector<float> hpts(4 * NHOST, 1.0f);
    // (the large image: float masks up to M = 12, uint8 up to 32 -- pages nobody touches)
    const size_t mask_bytes = big ? std::max((size_t)FMAX * 32 * hw, (size_t)FMAX * 12 * hw * 4) + 64 : (size_t)FMAX * 32 * hw * 4 + 64;
    char *dmasks = D.get<char>(mask_bytes);
    std::vector<char> hmasks(big ? 1 : mask_bytes, 1);
    int32_t *drects = D.get<int32_t>((size_t)FMAX * 32 * 4);
    std::vector<int32_t> hrects((size_t)FMAX * 32 * 4, 3);
    double *dcorners = D.get<double>(24 * 2 * FMAX);
    lpf_outputs od, oh;
    fill_outputs(D, od, NMAX, FMAX, 32, 2 * FMAX, 1000, 1);
    fill_outputs(D, oh, NHOST, FMAX, 32, 2 * FMAX, 1000, 0);
    static const int Ms[4] = {0, 5, 12, 32}, devs[5] = {0, 1, 2, 1, 2};
    // (the host-memory runs' staging at its largest first: a buffer that has to grow drains the pipeline, box job and all, and when that
    //  happens depends on how the staging is cut into buffers -- not on what this section is about)
    for (int sh = 0; sh < 2 && !big; ++sh) {
        const int64_t off[4] = {0, shapes[sh].n / 2, shapes[sh].n, shapes[sh].n};
        const int32_t boff[4] = {0, 2, 4, 6};
        CHECK(lpf_set_masks_u8(c, (const uint8_t *)hmasks.data(), shapes[sh].F, 32, 1, 0) == LPF_OK);
        CHECK(lpf_set_boxes_ex(c, dcorners, 2, boff, shapes[sh].F, 1) == LPF_OK);
        CHECK(lpf_run_batch(c, hpts.data(), off, shapes[sh].F, 0, &oh) == LPF_OK);
    }
    int combo = 0;
    for (int kind = 0; kind < 4; ++kind)                     // uint8, float under binarize 0 / 1 / 2
    for (int dv = big ? 1 : 0; dv < 5; ++dv)                 // host, copied, lent, copied and lent off the 16-byte boundary
    for (int with_rects = 0; with_rects < 2; ++with_rects)
    for (int erode = 0; erode < 2; ++erode)
    for (int sh = 0; sh < nshape; ++sh)
    for (int mi = 0; mi < 4; ++mi)
    for (int new_boxes = 1; new_boxes >= 0; --new_boxes) {
        const int M = Ms[mi], on_device = devs[dv], F = shapes[sh].F;
        const size_t esz = kind ? 4 : 1;
        if (big && kind && M > 12) continue;
        int64_t off[17];
        int32_t boff[17];
        off[0] = 0; boff[0] = 0;
        for (int f = 0; f < F; ++f) {
            off[f + 1] = (F == 3 && f == 1) ? off[f] : f == F - 1 ? shapes[sh].n : off[f] + shapes[sh].n / F;     // (an empty frame among three)
            boff[f + 1] = boff[f] + 2;
        }
        // (host masks go into scratch set 0, where only an in-order run looks for them)
        if (mode && !on_device && sh >= 2) continue;
        const bool host_run = !big && sh < 2 && (combo % 5 == 0 || (mode && !on_device));
        ++combo;
        if (with_rects && M > 0) CHECK(lpf_set_mask_rects(c, on_device ? drects : hrects.data(), on_device ? 1 : 0, F, M) == LPF_OK);
        const char *m = (on_device ? dmasks : hmasks.data()) + (dv >= 3 ? esz : 0);
        if (kind == 0) CHECK(lpf_set_masks_u8(c, (const uint8_t *)m, F, M, erode, on_device) == LPF_OK);
        else CHECK(lpf_set_masks_f32(c, (const float *)m, F, M, kind - 1, erode, on_device) == LPF_OK);
        if (new_boxes) CHECK(lpf_set_boxes_ex(c, dcorners, 2, boff, F, 1) == LPF_OK);
        if (host_run) CHECK(lpf_run_batch(c, hpts.data(), off, F, 0, &oh) == LPF_OK);
        else CHECK(lpf_run_batch(c, pts, off, F, 1, &od) == LPF_OK);
    }
    int64_t st[8];
    CHECK(lpf_get_stats(c, st, 8, 0) == LPF_OK);
    fprintf(stderr, "  mask sources, mode %d, %d x %d: %d runs, drains %lld, step launches %lld, box jobs alone %lld / riding %lld\n", mode, W, H, combo,
            (long long)st[1], (long long)st[3], (long long)st[4], (long long)st[5]);
    CHECK(lpf_sync(c) == LPF_OK);
    lpf_destroy(c);
    g_ctx = nullptr;
}

// Masks that are set but not packed when something else happens to the context: a mode switch, a camera of another size, a read or a
// replacement of the label image, masks set for no frames, a graph capture, a run that cannot be fused; and, in mode 4, tiles and a
// riding pack that do not go together in one launch (tiles that read masks themselves, or label elements of another size).
static void mask_transitions()
{
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(&c, 0) == LPF_OK);
    g_ctx = c;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    Dev D;
    const int F = 2, M = 5;
    const size_t hw = (size_t)W * H;
    const int64_t sparse[F + 1] = {0, 900, 1800}, dense[F + 1] = {0, 20000, 40000};
    float *pts = D.get<float>(4 * 40000);
    std::vector<float> hpts(4 * 40000, 1.0f);
    uint8_t *masks = D.get<uint8_t>((size_t)F * 32 * hw);
    float *fmasks = D.get<float>((size_t)F * 32 * hw);
    int32_t *drects = D.get<int32_t>((size_t)F * 32 * 4);
    std::vector<uint32_t> img((size_t)F * hw);
    lpf_outputs od, oh;
    fill_outputs(D, od, 40000, F, 32, 1, 1000, 1);
    fill_outputs(D, oh, 40000, F, 32, 1, 1000, 0);
    for (int mode = 2; mode <= 4; mode += 2) {
        // serial masks left unpacked, then the switch: packed on the switch, read by the first pipelined run
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_set_pipelined(c, mode) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, sparse, F, 1, &od) == LPF_OK);
        // lent masks of the pipelined context: read back (packed for it), then a run
        CHECK(lpf_set_masks_f32(c, fmasks, F, M, 1, 0, 2) == LPF_OK);
        CHECK(lpf_get_label_image(c, img.data(), 0) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, sparse, F, 1, &od) == LPF_OK);
        // ... a run through host memory: packed now, in order
        CHECK(lpf_set_mask_rects(c, drects, 1, F, M) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_run_batch(c, hpts.data(), sparse, F, 0, &oh) == LPF_OK);
        // ... tiles that read the masks themselves, then a dense run whose pack would ride beside them (mode 4: drained first), then
        //     dense runs with label elements of 1, 2, 4 and 1 bytes
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, sparse, F, 1, &od) == LPF_OK);
        static const int Ms[4] = {5, 12, 32, 5};
        for (int k = 0; k < 4; ++k) {
            CHECK(lpf_set_masks_u8(c, masks, F, Ms[k], 0, 2) == LPF_OK);
            CHECK(lpf_run_batch(c, pts, dense, F, 1, &od) == LPF_OK);
        }
        // ... a label image in their place: the lent masks stay on record and the next run still takes them (as it is today)
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_get_label_image(c, img.data(), 0) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_set_label_image(c, img.data(), F, M, 0) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, sparse, F, 1, &od) == LPF_OK);
        // ... masks for no frames: the run has no masks, the lent ones stay on record and are packed by it (as it is today)
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, nullptr, 0, 0, 0, 2) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, sparse, F, 1, &od) == LPF_OK);
        // ... a camera of another size forgets them: a run without masks, then back
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_set_camera(c, T16, K9, W / 2, H, 0, 50) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, sparse, F, 1, &od) == LPF_OK);
        CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
        // ... and the switch back with lent masks waiting: packed on the switch, read by the serial run
        CHECK(lpf_set_masks_f32(c, fmasks, F, M, 2, 0, 2) == LPF_OK);
        CHECK(lpf_set_pipelined(c, 0) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, sparse, F, 1, &od) == LPF_OK);
        // serial masks left unpacked: read back, replaced by a label image, forgotten with the camera's size
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_get_label_image(c, img.data(), 0) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_set_label_image(c, img.data(), F, M, 0) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, sparse, F, 1, &od) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, nullptr, 0, 0, 0, 2) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, sparse, F, 1, &od) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
        CHECK(lpf_set_camera(c, T16, K9, W / 2, H, 0, 50) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, sparse, F, 1, &od) == LPF_OK);
        CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
        // ... and captured into a graph: the tiles of the captured run read the lent masks themselves
        for (int k = 0; k < 2; ++k) {                      // (single frames: no tables to upload inside the capture)
            if (k) CHECK(lpf_graph_begin(c) == LPF_OK);
            CHECK(lpf_set_masks_u8(c, masks, 1, M, 0, 2) == LPF_OK);
            CHECK(lpf_run(c, pts, 900, 1, &od) == LPF_OK);
            CHECK(lpf_set_masks_u8(c, masks, 1, M, 0, 2) == LPF_OK);
            CHECK(lpf_run(c, pts, 20000, 1, &od) == LPF_OK);
        }
        lpf_graph *g = nullptr;
        CHECK(lpf_graph_end(c, &g) == LPF_OK && g);
        CHECK(lpf_graph_launch(c, g) == LPF_OK);
        lpf_graph_destroy(g);
    }
    lpf_destroy(c);
    g_ctx = nullptr;
}

// the packs of lpf_run_cams, lpf_run_wide and lpf_depth_maps for every mask rule and label width: uint8 and float masks under each of
// the three rules, with and without erosion, 5 / 12 / 32 masks per camera (one label element type per pass), passes of few points
// (512-point tiles) and of more than 917 504 (1024-point tiles)
static void pack_forms()
{
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(&c, 0) == LPF_OK);
    g_ctx = c;
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    Dev D;
    const size_t hw = (size_t)W * H;
    const int64_t NMAX = 1000000;
    float *pts = D.get<float>(4 * NMAX);
    char *dmasks = D.get<char>(32 * hw * 4 + 64);
    int32_t *drects = D.get<int32_t>(32 * 4);
    static const int Ms[3] = {5, 12, 32};
    for (int kind = 0; kind < 4; ++kind)
    for (int erode = 0; erode < 3; ++erode)
    for (int mi = 0; mi < 3; ++mi)
    for (int shape = 0; shape < 2; ++shape)
    for (int unaligned = 0; unaligned < 2; ++unaligned) {
        const int64_t off[2] = {0, shape ? NMAX : 3000};
        lpf_cam_input cam;
        memset(&cam, 0, sizeof cam);
        memcpy(cam.T_velo_to_rect, T16, sizeof T16); memcpy(cam.K, K9, sizeof K9); cam.W = W; cam.H = H; cam.depth_max_excl = 50;
        cam.masks.masks = dmasks + (unaligned ? (kind ? 4 : 1) : 0); cam.masks.rects = erode ? nullptr : drects; cam.masks.M = Ms[mi];
        cam.masks.f32 = kind != 0; cam.masks.binarize = kind ? kind - 1 : 0; cam.masks.erode_iters = erode; cam.masks.on_device = 1;
        lpf_outputs o;
        fill_outputs(D, o, 1, 1, 1, 1, 100, 1);
        o.uv = nullptr; o.label_bits = nullptr; o.valid_idx = nullptr; o.uv_valid = nullptr; o.label_valid = nullptr;      // (summaries and lists' counts only)
        o.inst_idx = nullptr; o.count_mb = nullptr;
        CHECK(lpf_run_cams(c, pts, off, 1, 1, &cam, 1, &o) == LPF_OK);
        if (shape || unaligned) continue;
        lpf_wide_outputs w1;
        memset(&w1, 0, sizeof w1);
        w1.n_valid = D.get<int64_t>(1); w1.on_device = 1;
        CHECK(lpf_run_wide(c, pts, off, 1, 1, &cam.masks, &w1) == LPF_OK);
        lpf_depth_maps_outputs dm;
        memset(&dm, 0, sizeof dm);
        dm.cap = 100; dm.pix = D.get<int64_t>(100); dm.car_off = D.get<int64_t>(Ms[mi] + 1); dm.need = D.get<int64_t>(1); dm.on_device = 1;
        CHECK(lpf_depth_maps(c, pts, off, 1, 1, &cam.masks, &dm) == LPF_OK);
    }
    lpf_destroy(c);
    g_ctx = nullptr;
}

// The box state's transitions (lpf_ctx::Boxes), by what the interface shows of them: a run of another frame count is refused while
// boxes are in force ("boxes were set for ..."), and lpf_get_stats counts the box jobs ([4] launched alone, [5] riding in a step launch).
static void box_transitions()
{
    Dev D;
    const int F = 2, M = 2;
    const int64_t off[F + 1] = {0, 3000, 6000}, off1[2] = {0, 3000};
    const int32_t boff[F + 1] = {0, 70, 73}, bad0[F + 1] = {1, 70, 73}, desc[F + 1] = {0, 70, 3};     // (two 64-box words in frame 0)
    float *pts = D.get<float>(4 * off[F]);
    uint8_t *masks = D.get<uint8_t>((size_t)F * M * W * H);
    double *corners = D.get<double>(24 * boff[F]);
    std::vector<double> hcorners(24 * boff[F], 0.5);
    lpf_outputs o;
    fill_outputs(D, o, off[F], F, M, boff[F], 500, 1);
    lpf_wide_input wi;
    memset(&wi, 0, sizeof wi);
    wi.masks = masks; wi.M = M; wi.on_device = 1;
    lpf_wide_outputs ow;
    fill_wide_outputs(D, ow, off[F], F, M, boff[F], 500, 1);
    double K2[9];
    memcpy(K2, K9, sizeof K2);
    K2[0] = 300.0; K2[2] = 60.0;                                 // same W x H, another K
    int64_t st[8];
    auto jobs = [&]() { CHECK(lpf_get_stats(g_ctx, st, 8, 1) == LPF_OK); return st[4] + st[5]; };     // box jobs since the last look
    auto in_force = [&](lpf_ctx *c) {                            // boxes for F frames are in force: a run of one frame is refused
        return lpf_run_wide(c, pts, off1, 1, 1, &wi, &ow) == LPF_ERR_STATE && err_is("boxes were set for 2 frames, run_wide has 1");
    };
    for (int mode = 0; mode <= 4; mode += 2) {
        lpf_ctx *c = nullptr;
        CHECK(lpf_create(&c, 0) == LPF_OK);
        g_ctx = c;
        CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
        CHECK(lpf_set_pipelined(c, mode) == LPF_OK);
        auto run = [&]() {
            CHECK(lpf_set_masks_u8(c, masks, F, M, 0, 2) == LPF_OK);
            CHECK(lpf_run_batch(c, pts, off, F, 1, &o) == LPF_OK);
        };
        // set boxes, run -- four times round the ring: every set's job is launched once, with its run; the pipeline is never drained
        jobs();
        for (int r = 0; r < 16; ++r) {
            CHECK(lpf_set_boxes_ex(c, r & 1 ? corners : hcorners.data(), r & 1 ? 2 : 0, boff, F, r & 1) == LPF_OK);
            run();
        }
        CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK && st[4] == 0 && st[5] == 16 && st[1] == 0);
        // boxes set twice before a run: the second call rewrites the set of the first (no run has read it), one job
        CHECK(lpf_set_boxes_ex(c, hcorners.data(), 0, boff, F, 1) == LPF_OK);
        CHECK(lpf_set_boxes_ex(c, hcorners.data(), 0, boff, F, 0) == LPF_OK);
        run();
        CHECK(jobs() == 1);
        // a run with the tables as they are: no job
        run();
        CHECK(jobs() == 0);
        // the camera changes, same W x H: the boxes stay in force and their tables are not built again
        CHECK(lpf_set_camera(c, T16, K2, W, H, 0, 50) == LPF_OK);
        CHECK(in_force(c));
        run();
        CHECK(jobs() == 0);
        CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
        CHECK(lpf_run_wide(c, pts, off, F, 1, &wi, &ow) == LPF_OK);
        CHECK(jobs() == 0);
        // a job that waits is launched by lpf_set_camera's drain, in the old camera, and not again by the run
        CHECK(lpf_set_boxes_cam0(c, corners, 2, boff, F, T16, 1, 1, nullptr, nullptr, nullptr, nullptr) == LPF_OK);
        CHECK(lpf_set_camera(c, T16, K2, W, H, 0, 50) == LPF_OK);
        CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK && st[4] == 1 && st[5] == 0);
        run();
        CHECK(jobs() == 0);
        // refused arguments leave the earlier boxes in force
        CHECK(lpf_set_boxes_ex(c, hcorners.data(), 0, bad0, F, 1) == LPF_ERR_ARG && in_force(c));
        CHECK(lpf_set_boxes_ex(c, hcorners.data(), 0, desc, F, 1) == LPF_ERR_ARG && in_force(c));
        CHECK(lpf_set_boxes_ex(c, nullptr, 0, boff, F, 1) == LPF_ERR_ARG && in_force(c));
        CHECK(lpf_set_boxes_cam0(c, corners, 2, boff, F, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr) == LPF_ERR_ARG && in_force(c));
        run();
        CHECK(jobs() == 0);
        // lpf_run_cams builds its cameras' tables in sets of its own: the context's boxes stay in force, with their tables
        lpf_cam_input cam;
        memset(&cam, 0, sizeof cam);
        memcpy(cam.T_velo_to_rect, T16, sizeof T16); memcpy(cam.K, K2, sizeof K2); cam.W = W; cam.H = H; cam.depth_max_excl = 50;
        cam.masks = wi; cam.corners_velo = hcorners.data(); cam.box_off = boff; cam.oriented = 1;
        CHECK(lpf_run_cams(c, pts, off, F, 1, &cam, 1, &o) == LPF_OK);
        CHECK(lpf_get_stats(c, st, 8, 1) == LPF_OK && st[4] == 1 && st[5] == 0);      // the camera's own job
        CHECK(in_force(c));
        run();
        CHECK(jobs() == 0);
        // F == 0 after boxes were set: none in force, a run of any frame count goes through and launches no job
        CHECK(lpf_set_boxes_ex(c, nullptr, 0, nullptr, 0, 1) == LPF_OK);
        CHECK(lpf_set_masks_u8(c, masks, 1, M, 0, 2) == LPF_OK);
        CHECK(lpf_run_batch(c, pts, off1, 1, 1, &o) == LPF_OK);
        run();
        CHECK(jobs() == 0);
        // a camera of another size drops the boxes of every set
        CHECK(lpf_set_boxes_ex(c, hcorners.data(), 0, boff, F, 1) == LPF_OK);
        CHECK(lpf_set_camera(c, T16, K9, W / 2, H, 0, 50) == LPF_OK);
        CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
        CHECK(!in_force(c));
        CHECK(lpf_sync(c) == LPF_OK);
        lpf_destroy(c);
        g_ctx = nullptr;
    }
}

// the launches so far and their hash; the hash of the copies and memsets since the section before (the reader's worker threads copy in
// an order of their own, so the hash of "reader, box_files" differs from run to run -- every other section's is a constant)
static void section(const char *name)
{
    fprintf(stderr, "  trace after %-24s %lld launches, hash %016llx, its copies %016llx\n", name, fake_hip_launches(), fake_hip_trace_hash(), fake_hip_copy_hash(1));
}

int main(int argc, char **argv)
{
    const char *tmp = argc > 1 ? argv[1] : "/tmp";
    const int runs = argc > 2 ? atoi(argv[2]) : 12000;
    argument_errors();
    host_memory_runs();
    section("host_memory_runs");
    wide_and_multicam_runs();
    section("wide_and_multicam_runs");
    table_key();
    ring_of_small_uploads();
    section("table_key, ring");
    pipelined_streams(2, runs, W, H);
    pipelined_streams(4, runs, W, H);
    pipelined_streams(2, runs / 8, 1408, 376);
    pipelined_streams(4, runs / 8, 1408, 376);
    pipelined_streams(0, runs / 8, 1408, 376);               // in order
    section("pipelined_streams");
    graphs();
    section("graphs");
    reader(tmp);
    box_files(tmp);
    section("reader, box_files");
    for (int mode = 0; mode <= 4; mode += 2) {
        mask_sources(mode, W, H);
        mask_sources(mode, 1408, 376);                       // (large sparse launches: the rectangles' candidate grid ahead of the tiles, riding in mode 4)
    }
    section("mask_sources");
    mask_transitions();
    section("mask_transitions");
    pack_forms();
    section("pack_forms");
    box_transitions();
    section("box_transitions");
    return drive_finish("drive", false);
}
