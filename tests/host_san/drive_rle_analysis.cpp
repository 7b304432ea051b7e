// drive_rle_analysis.cpp -- drives the HOST side of lpf_depth_maps_rle and lpf_first_match_rle (lpf_api.hip compiled --offload-host-only
// against fake_hip.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: every refusal of both calls with its message and nothing
// queued -- a bad run in the LAST frame of a batch that spans several ranges among them --, M = 0 and masks without runs (no decode
// launch), batches whose label planes exceed the 256 MiB staging bound (several ranges, each with its own slice of the runs), growing
// then shrinking calls, and a pipelined context with a narrow run owed.  The caller's arrays AND structs live in exactly-sized heap
// blocks that are scribbled over and freed as soon as the call has returned.  ONLY run-length masks are run here, so that
// tests/test_host_sanitized_rle_analysis.py can say from the FAKE_HIP_TRACE file: lpf_fm_count_planes and lpf_dm_raster's planes
// instantiation ran, no dense count ran, no dense mask was copied (each successful call prints the bytes its dense twin would have
// copied: "dense-bytes N").  The multi-range section stands between two marker memsets (mark()) in the trace.  Results are checked on
// the GPU by tests/test_gpu_rle_analysis.py.
#include "drive_common.h"
#include <climits>

static const int W = 37, H = 23, HW = W * H;                 // the context's camera
static const int W1 = 30, H1 = 20, HW1 = W1 * H1;            // masks of their own, smaller size (first match)
static const int BW = 1408, BH = 376, BHW = BW * BH;         // the large image of the multi-range section
static const int NPTS = 1001, FMAX = 17;

static void mark()                                           // "memset 7": a size no call of the library has
{
    static char buf[8];
    hipMemsetAsync(buf, 0, 7, nullptr);
}

// drive_common.h's, with this driver's image as the default
static Rle simple(int F, int M, int runs_per_mask, int length = 3, int hw = HW);
static bool in_force(lpf_ctx *c, int F, int hw = HW);

static std::vector<float> g_pts(4 * (size_t)NPTS * FMAX, 1.0f);
static int64_t g_off[FMAX + 1];

// lpf_depth_maps_rle with k as its masks (F: the call's frames); the arrays and the struct are gone when it returns
static int depth_maps(lpf_ctx *c, const Rle &k, int F, long long hw = HW, long long cap = 50)
{
    Dev D;
    const int M = k.M > 0 && k.M <= LPF_MAX_MASKS_WIDE ? k.M : 1;
    lpf_depth_maps_outputs *o = (lpf_depth_maps_outputs *)malloc(sizeof(lpf_depth_maps_outputs));
    memset(o, 0, sizeof *o);
    const size_t rows = (size_t)F * (size_t)(cap > 0 ? cap : 1);
    o->cap = cap; o->pix = D.get<int64_t>(rows); o->depth = D.get<double>(rows); o->point_idx = D.get<int64_t>(rows);
    o->car_off = D.get<int64_t>((size_t)F * (M + 1)); o->need = D.get<int64_t>(F); o->overflow = D.get<int32_t>(F);
    Held h(k);
    const int rc = lpf_depth_maps_rle(c, g_pts.data(), g_off, F, 0, h.in, o);
    h.release();
    memset(o, 0xEE, sizeof *o);
    free(o);
    if (rc == LPF_OK && k.M > 0) fprintf(stderr, "dense-bytes %lld\n", (long long)F * k.M * hw);
    return rc;
}

// lpf_first_match_rle with k as its masks at mh x mw; colours when there are masks; lists: every list, or the counts only
static int first_match(lpf_ctx *c, const Rle &k, int F, int mh = H, int mw = W, bool lists = true, int in_reserved = 0, bool no_counts = false)
{
    Dev D;
    const int M = k.M > 0 && k.M <= LPF_MAX_MASKS_WIDE ? k.M : 1;
    const size_t n = (size_t)F * NPTS;
    lpf_first_match_outputs *o = (lpf_first_match_outputs *)malloc(sizeof(lpf_first_match_outputs));
    memset(o, 0, sizeof *o);
    double *colors = (double *)malloc((size_t)F * M * 3 * sizeof(double));
    for (size_t i = 0; i < (size_t)F * M * 3; ++i) colors[i] = 0.25;
    if (lists) {
        o->first_mask = D.get<int32_t>(n); o->car_idx = D.get<int64_t>(n); o->car_mask = D.get<int32_t>(n); o->car_xyz = D.get<float>(3 * n);
        o->car_rgb = D.get<double>(3 * n); o->bg_idx = D.get<int64_t>(n); o->bg_xyz = D.get<float>(3 * n);
        o->mask_count = D.get<int64_t>((size_t)F * M);
    }
    o->n_valid = D.get<int64_t>(F);
    if (!no_counts) { o->n_car = D.get<int64_t>(F); o->n_bg = D.get<int64_t>(F); }
    Held h(k);
    lpf_first_match_rle_input *in = (lpf_first_match_rle_input *)malloc(sizeof(lpf_first_match_rle_input));
    memset(in, 0, sizeof *in);
    in->masks = h.in; in->colors = colors; in->mh = mh; in->mw = mw; in->reserved = in_reserved;
    const int rc = lpf_first_match_rle(c, g_pts.data(), g_off, F, 0, in, o);
    h.release();
    memset(in, 0xEE, sizeof *in); memset(o, 0xEE, sizeof *o); memset(colors, 0xEE, (size_t)F * M * 3 * sizeof(double));
    free(in); free(o); free(colors);
    if (rc == LPF_OK && k.M > 0) fprintf(stderr, "dense-bytes %lld\n", (long long)F * k.M * mh * mw);
    return rc;
}

// F frames of M one-run masks on the large image: frame f, mask m = pixels [(f * M + m) * 64, + 1 + f)
static Rle large(int F, int M)
{
    Rle k;
    k.F = F; k.M = M;
    k.off.push_back(0);
    for (int f = 0; f < F; ++f)
        for (int m = 0; m < M; ++m) {
            k.runs.push_back(((f * M + m) * 64) % (BHW - 64)); k.runs.push_back(1 + f);
            k.off.push_back((int64_t)k.runs.size() / 2);
        }
    return k;
}

static void refusals(lpf_ctx *c)
{
    {                                                        // the narrow state every call below must leave alone
        const Rle n = simple(2, 3, 2);
        Held h(n);
        CHECK(lpf_set_masks_rle(c, h.in) == LPF_OK);
        h.release();
        CHECK(in_force(c, 2));
    }
    CHECK(depth_maps(c, simple(1, 5, 2), 1) == LPF_OK);      // (the calls' buffers exist; these are fine as they are)
    CHECK(first_match(c, simple(1, 5, 2), 1) == LPF_OK);
    const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
    char want[512];
    Rle k;

    // ---- lpf_depth_maps_rle
    k = simple(2, 5, 2);
    CHECK(depth_maps(c, k, 1) == LPF_ERR_ARG && err_is("depth_maps_rle: the run-length masks say F=2, the call has F=1"));
    k = simple(1, LPF_MAX_MASKS_WIDE + 1, 1);
    CHECK(depth_maps(c, k, 1) == LPF_ERR_ARG && err_is("depth_maps_rle: M=257 masks per frame, lpf_depth_maps_rle takes 0 .. LPF_MAX_MASKS_WIDE = 256"));
    k = simple(1, 5, 2); k.M = -1;
    CHECK(depth_maps(c, k, 1) == LPF_ERR_ARG && err_is("depth_maps_rle: M=-1 masks per frame, lpf_depth_maps_rle takes 0 .. LPF_MAX_MASKS_WIDE = 256"));
    k = simple(1, 5, 2); k.erode = -1;
    CHECK(depth_maps(c, k, 1) == LPF_ERR_ARG && err_is("depth_maps_rle: erode_iters=-1 reserved=0"));
    k = simple(1, 5, 2); k.reserved = 7;
    CHECK(depth_maps(c, k, 1) == LPF_ERR_ARG && err_is("depth_maps_rle: erode_iters=0 reserved=7"));
    k = simple(1, 5, 2);
    CHECK(depth_maps(c, k, 1, HW, -1) == LPF_ERR_ARG && strncmp(lpf_last_error(c), "depth_maps_rle: cap=-1 pix=", 27) == 0);
    k = simple(1, 5, 2); k.off[0] = 1;
    CHECK(depth_maps(c, k, 1) == LPF_ERR_ARG && err_is("depth_maps_rle: run_off[0]=1 (must be 0)"));
    k = simple(2, 3, 2); k.off[5] = 7;
    CHECK(depth_maps(c, k, 2) == LPF_ERR_ARG && err_is("depth_maps_rle: run_off decreases at frame 1 mask 1 (7 after 8)"));
    k = simple(1, 2, 1); k.off.clear();
    CHECK(depth_maps(c, k, 1) == LPF_ERR_ARG && err_is("depth_maps_rle: run_off=NULL with F=1 M=2"));
    k = simple(1, 2, 1); k.runs.clear();
    CHECK(depth_maps(c, k, 1) == LPF_ERR_ARG && err_is("depth_maps_rle: runs=NULL with 2 runs"));
    struct Bad { int32_t start, length; } bad[] = {{-1, 3}, {5, -1}, {HW - 2, 3}, {HW, 1}, {INT32_MAX, INT32_MAX}, {0, HW + 1}, {INT32_MIN, 0}};
    for (const Bad &b : bad) {
        k = simple(2, 40, 2);                                // run 1 of frame 1, mask 33: global run 2 * (40 + 33) + 1
        const int g = 2 * (40 + 33) + 1;
        k.runs[2 * g] = b.start; k.runs[2 * g + 1] = b.length;
        snprintf(want, sizeof want, "depth_maps_rle: frame 1 mask 33 run 1: start=%d length=%d (0 <= start, 0 <= length, start + length <= W*H = %d)",
                 b.start, b.length, HW);
        CHECK(depth_maps(c, k, 2) == LPF_ERR_ARG && err_is(want));
    }
    {
        Dev D;
        lpf_depth_maps_outputs o;
        memset(&o, 0, sizeof o);
        o.car_off = D.get<int64_t>(6); o.need = D.get<int64_t>(1);
        CHECK(lpf_depth_maps_rle(c, g_pts.data(), g_off, 1, 0, nullptr, &o) == LPF_ERR_ARG &&
              strncmp(lpf_last_error(c), "depth_maps_rle: masks=", 22) == 0);
    }

    // ---- lpf_first_match_rle
    k = simple(2, 5, 2);
    CHECK(first_match(c, k, 1) == LPF_ERR_ARG && err_is("first_match_rle: the run-length masks say F=2, the call has F=1"));
    k = simple(1, LPF_MAX_MASKS_WIDE + 1, 1);
    CHECK(first_match(c, k, 1) == LPF_ERR_ARG && err_is("first_match_rle: M=257 masks per frame, lpf_first_match_rle takes 0 .. LPF_MAX_MASKS_WIDE = 256"));
    k = simple(1, 5, 2); k.erode = 1;
    CHECK(first_match(c, k, 1) == LPF_ERR_ARG && err_is("first_match_rle: erode_iters=1 (the first-mask labelling has no erosion: 0)"));
    k = simple(1, 5, 2); k.reserved = 7;
    CHECK(first_match(c, k, 1) == LPF_ERR_ARG && err_is("first_match_rle: reserved=0, the masks' reserved=7 (both 0)"));
    k = simple(1, 5, 2);
    CHECK(first_match(c, k, 1, H, W, true, 3) == LPF_ERR_ARG && err_is("first_match_rle: reserved=3, the masks' reserved=0 (both 0)"));
    CHECK(first_match(c, k, 1, 0, W) == LPF_ERR_ARG && err_is("first_match_rle: mh=0 mw=37 (with M > 0 both are > 0)"));
    CHECK(first_match(c, k, 1, H, -2) == LPF_ERR_ARG && err_is("first_match_rle: mh=23 mw=-2 (with M > 0 both are > 0)"));
    CHECK(first_match(c, k, 1, H, W, false, 0, true) == LPF_ERR_ARG && strncmp(lpf_last_error(c), "first_match_rle: n_car=", 23) == 0);
    // a run one pixel past mh x mw = 20 x 30 that fits the camera's 23 x 37 image: the masks' OWN size is the bound
    k = simple(1, 5, 2, 3, HW1);
    k.runs[0] = HW1 - 2;
    snprintf(want, sizeof want, "first_match_rle: frame 0 mask 0 run 0: start=%d length=3 (0 <= start, 0 <= length, start + length <= W*H = %d)",
             HW1 - 2, HW1);
    CHECK(first_match(c, k, 1, H1, W1) == LPF_ERR_ARG && err_is(want));
    CHECK(fake_hip_launches() == l0 && fake_hip_copies() == c0);     // nothing was queued by any refusal so far
    CHECK(first_match(c, k, 1, H, W) == LPF_OK);             // (the same runs on masks of the camera's size are fine)
    const long long l1 = fake_hip_launches(), c1 = fake_hip_copies();
    k = simple(2, 3, 2); k.off[5] = 7;
    CHECK(first_match(c, k, 2) == LPF_ERR_ARG && err_is("first_match_rle: run_off decreases at frame 1 mask 1 (7 after 8)"));
    {
        Dev D;
        lpf_first_match_outputs o;
        memset(&o, 0, sizeof o);
        o.n_car = D.get<int64_t>(1); o.n_bg = D.get<int64_t>(1);
        lpf_first_match_rle_input in;
        memset(&in, 0, sizeof in);
        in.mh = H; in.mw = W;
        CHECK(lpf_first_match_rle(c, g_pts.data(), g_off, 1, 0, &in, &o) == LPF_ERR_ARG &&
              strncmp(lpf_last_error(c), "first_match_rle: in=", 20) == 0);
    }
    // ... nor by these, and the narrow masks are still in force
    CHECK(fake_hip_launches() == l1 && fake_hip_copies() == c1);
    CHECK(in_force(c, 2));

    // ---- a bad run in the LAST frame of a batch that spans several ranges: refused before the first range is enqueued
    CHECK(lpf_set_camera(c, T16, K9, BW, BH, 0, 50) == LPF_OK);
    const long long l2 = fake_hip_launches(), c2 = fake_hip_copies();
    k = large(FMAX, 256);
    k.runs[2 * (FMAX * 256 - 1)] = BHW - 3; k.runs[2 * (FMAX * 256 - 1) + 1] = 4;
    snprintf(want, sizeof want, "depth_maps_rle: frame 16 mask 255 run 0: start=%d length=4 (0 <= start, 0 <= length, start + length <= W*H = %d)",
             BHW - 3, BHW);
    CHECK(depth_maps(c, k, FMAX, BHW) == LPF_ERR_ARG && err_is(want));
    snprintf(want, sizeof want, "first_match_rle: frame 16 mask 255 run 0: start=%d length=4 (0 <= start, 0 <= length, start + length <= W*H = %d)",
             BHW - 3, BHW);
    CHECK(first_match(c, k, FMAX, BH, BW) == LPF_ERR_ARG && err_is(want));
    CHECK(fake_hip_launches() == l2 && fake_hip_copies() == c2);
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
}

template <typename Call> static long long launches_of(Call &&call)
{
    const long long l0 = fake_hip_launches();
    CHECK(call() == LPF_OK);
    return fake_hip_launches() - l0;
}

static void no_decode(lpf_ctx *c)
{
    // masks without runs, and runs that are all empty: one launch fewer than the same masks with runs -- the decode
    for (int which = 0; which < 2; ++which) {
        auto run = [&](const Rle &k) { return launches_of([&] { return which ? first_match(c, k, 2) : depth_maps(c, k, 2); }); };
        const long long with_runs = run(simple(2, 40, 2)), none = run(simple(2, 40, 0));
        CHECK(with_runs - none == 1);
        CHECK(run(simple(2, 40, 2, 0)) == none);
        Rle k = Rle(); k.F = 2; k.M = 0; k.off = {0};        // M = 0, with run_off's one entry or without it
        const long long m0 = run(k);
        k.off.clear();
        CHECK(run(k) == m0 && m0 <= none);
        if (!which) {                                        // erosion: every iteration a launch of its own; the 1 x 1 element is the identity
            k = simple(2, 40, 2); k.erode = 2;
            CHECK(run(k) == with_runs + 2);
            k = simple(2, 40, 0); k.erode = 2;
            CHECK(run(k) == none);
            CHECK(lpf_set_erosion_element(c, 5) == LPF_OK);
            k = simple(2, 40, 2); k.erode = 2;
            CHECK(run(k) == with_runs + 2);
            CHECK(lpf_set_erosion_element(c, 1) == LPF_OK);
            CHECK(run(k) == with_runs);
            CHECK(lpf_set_erosion_element(c, 3) == LPF_OK);
        }
    }
}

// batches whose label planes exceed the 256 MiB staging bound, between markers in the trace
static void several_ranges(lpf_ctx *c)
{
    CHECK(lpf_set_camera(c, T16, K9, BW, BH, 0, 50) == LPF_OK);
    const Rle k = large(FMAX, 256);
    mark();
    fprintf(stderr, "section first_match\n");
    CHECK(first_match(c, k, FMAX, BH, BW) == LPF_OK);
    mark();
    fprintf(stderr, "section depth_maps\n");
    CHECK(depth_maps(c, k, FMAX, BHW, 400) == LPF_OK);
    mark();
    Rle e = large(FMAX, 256);                                // eroded: the planes ping-pong, so a range holds half as many frames
    e.erode = 1;
    CHECK(depth_maps(c, e, FMAX, BHW, 400) == LPF_OK);
    mark();
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
}

static void sizes(lpf_ctx *c)
{
    // M = 256, F = 3: shuffled order, overlaps and repeats, ragged with empty masks
    Rle big;
    big.F = 3; big.M = 256;
    big.off.push_back(0);
    unsigned s = 12345;
    for (int i = 0; i < big.F * big.M; ++i) {
        const int n = i % 3 == 0 ? 0 : 40 + i % 5;
        for (int j = 0; j < n; ++j) {
            s = s * 1664525u + 1013904223u;
            const int start = (int)((s >> 8) % HW), length = (int)((s >> 3) % (HW - start + 1));
            big.runs.push_back(start); big.runs.push_back(length);
        }
        big.off.push_back((int64_t)big.runs.size() / 2);
    }
    CHECK(first_match(c, big, 3) == LPF_OK);
    CHECK(depth_maps(c, big, 3) == LPF_OK);
    big.erode = 2;
    CHECK(depth_maps(c, big, 3, HW, 0) == LPF_OK);           // (cap 0: the counts only)
    // growing then shrinking calls on the same context; masks smaller and larger than the image
    for (int F : {1, 3, 2, 1})
        for (int M : {1, 33, 256, 40, 5}) {
            Rle k = simple(F, M, F + M % 7, 1 + M % 9);
            CHECK(first_match(c, k, F, H, W, M % 2 == 0) == LPF_OK);
            k.erode = M % 3;
            CHECK(depth_maps(c, k, F, HW, 10 * M) == LPF_OK);
            Rle k1 = simple(F, M, 2 + M % 5, 1 + M % 9, HW1);
            CHECK(first_match(c, k1, F, H1, W1) == LPF_OK);
            Rle k2 = simple(F, M, 2, 5, 4 * HW);
            CHECK(first_match(c, k2, F, 2 * H, 2 * W) == LPF_OK);
        }
    CHECK(first_match(c, simple(0, 5, 0), 0) == LPF_OK);     // F = 0
    CHECK(depth_maps(c, simple(0, 5, 0), 0) == LPF_OK);
}

// a pipelined context with a narrow run owed: the call launches what is owed and runs in order; the narrow masks stay in force
static void pipelined(lpf_ctx *c)
{
    for (int mode : {2, 4, 0}) {
        CHECK(lpf_set_pipelined(c, mode) == LPF_OK);
        Dev D;
        lpf_outputs o;
        memset(&o, 0, sizeof o);
        o.uv = D.get<int32_t>(2 * NPTS); o.label_bits = D.get<uint32_t>(NPTS); o.valid_idx = D.get<int64_t>(NPTS);
        o.inst_idx = D.get<int64_t>(100); o.inst_cap = 100; o.count_mb = D.get<int32_t>(32);
        o.summary = D.get<lpf_frame_summary>(1); o.uv_valid = D.get<int32_t>(2 * NPTS); o.label_valid = D.get<uint32_t>(NPTS);
        for (int it = 0; it < 3; ++it) {
            const Rle n = simple(1, 5 + 6 * it, 3);
            Held h(n);
            CHECK(lpf_set_masks_rle(c, h.in) == LPF_OK);
            h.release();
            CHECK(lpf_run_batch(c, g_pts.data(), g_off, 1, 0, &o) == LPF_OK);        // owed, in modes 2 / 4
            Rle k = simple(1, 40 + it, 3);
            CHECK(first_match(c, k, 1) == LPF_OK);
            CHECK(lpf_run_batch(c, g_pts.data(), g_off, 1, 0, &o) == LPF_OK);
            k.erode = it;
            CHECK(depth_maps(c, k, 1) == LPF_OK);
        }
        CHECK(lpf_sync(c) == LPF_OK);
    }
    CHECK(in_force(c, 1));
}

// the dense twins, on two frames WITHOUT points: no dense count or raster is launched, so this driver's trace stays run-length only
// (tests/test_host_sanitized_rle_analysis.py reads it so) while the host side stages the dense masks and walks every range
static int dense_call(lpf_ctx *c, bool fm)
{
    Dev D;
    const int F = 2, M = 3;
    static const int64_t empty[F + 1] = {0, 0, 0};
    uint8_t *masks = D.get<uint8_t>((size_t)F * M * HW);
    if (fm) {
        lpf_first_match_input in;
        lpf_first_match_outputs o;
        memset(&in, 0, sizeof in); memset(&o, 0, sizeof o);
        in.masks = masks; in.M = M; in.mh = H; in.mw = W;
        o.n_valid = D.get<int64_t>(F); o.n_car = D.get<int64_t>(F); o.n_bg = D.get<int64_t>(F); o.mask_count = D.get<int64_t>(F * M);
        return lpf_first_match(c, nullptr, empty, F, 0, &in, &o);
    }
    lpf_wide_input in;
    lpf_depth_maps_outputs o;
    memset(&in, 0, sizeof in); memset(&o, 0, sizeof o);
    in.masks = masks; in.M = M;
    o.cap = 10; o.pix = D.get<int64_t>(F * 10); o.car_off = D.get<int64_t>(F * (M + 1)); o.need = D.get<int64_t>(F);
    return lpf_depth_maps(c, nullptr, empty, F, 0, &in, &o);
}

// An allocation that fails inside lpf_depth_maps_rle / lpf_first_match_rle -- after the walk, which allocates nothing: every one of the
// call's allocations in turn, each on a fresh context (fake_hip_fail_malloc_after).  The call returns the allocation's error; the
// caller's arrays are scribbled over and freed (depth_maps / first_match above); then the SAME context runs both dense calls and both
// run-length calls: nothing of it may still point into those arrays
static void failed_allocations()
{
    lpf_ctx *outer = g_ctx;
    Rle e = simple(2, 3, 2);
    e.erode = 1;
    for (int which = 0; which < 2; ++which) {
        int failed = 0;
        for (int n = 0; n < 64; ++n) {
            lpf_ctx *c = nullptr;
            CHECK(lpf_create(&c, 0) == LPF_OK && c);
            g_ctx = c;
            CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
            fake_hip_fail_malloc_after(n);
            const int rc = which ? first_match(c, simple(2, 3, 2), 2) : depth_maps(c, e, 2);
            fake_hip_fail_malloc_after(-1);
            if (rc != LPF_OK) {
                ++failed;
                CHECK(rc == LPF_ERR_NOMEM && strncmp(lpf_last_error(c), "hipMalloc(", 10) == 0);
            }
            CHECK(dense_call(c, false) == LPF_OK);
            CHECK(dense_call(c, true) == LPF_OK);
            CHECK(depth_maps(c, e, 2) == LPF_OK);
            CHECK(first_match(c, simple(2, 3, 2), 2) == LPF_OK);
            lpf_destroy(c);
            g_ctx = outer;
            if (rc == LPF_OK) break;                         // (n allocations sufficed: the call has no more to fail)
        }
        CHECK(failed >= 4);                                  // (the tables, the planes, the run tables and the staging buffers at least)
    }
}

int main()
{
    for (int f = 0; f <= FMAX; ++f) g_off[f] = (int64_t)f * NPTS;
    lpf_ctx *c = drive_begin();
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    refusals(c);
    no_decode(c);
    several_ranges(c);
    sizes(c);
    pipelined(c);
    failed_allocations();
    lpf_destroy(c);
    return drive_finish("drive_rle_analysis", false);
}
