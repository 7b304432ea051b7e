// drive_rle_wide.cpp -- drives the HOST side of run-length masks in the wide and multi-camera passes (lpf_wide_input.f32 =
// LPF_MASKS_RLE in lpf_run_wide, lpf_run_cams, lpf_run_cams_wide; lpf_api.hip compiled --offload-host-only against fake_hip.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: every refusal of the three calls with its message and nothing queued, the calls that
// refuse the form (lpf_depth_maps, lpf_first_match) before they read `masks`, M = 0 and masks without runs (no decode launch), M = 256
// with F = 3, two run-length cameras in one pass, growing then shrinking calls, and a pipelined context with a narrow run owed.  The
// caller's arrays AND the lpf_rle_masks struct live in exactly-sized heap blocks that are scribbled over and freed as soon as the call
// has returned.  ONLY run-length masks (and cameras without masks) are run here, so that tests/test_host_sanitized_rle_wide.py can say
// from the FAKE_HIP_TRACE file: lpf_rle_decode_wide ran, no dense pack ran, no dense mask was copied (each successful call prints the
// bytes its dense twin would have copied: "dense-bytes N"), and erosion is the packed image's.  lpf_run_frame_wide is not driven: its job
// has no form field (its masks are uint8 device memory), so the form cannot be given to it.  Results are checked on the GPU by
// tests/test_gpu_wide_rle.py.
#include "drive_common.h"
#include <climits>

static const int W = 37, H = 23, HW = W * H;                 // the context's camera, and camera 0 of a camera pass
static const int W1 = 30, H1 = 20, HW1 = W1 * H1;            // camera 1: smaller
static const int NPTS = 1001;                                // (16 016 bytes per frame: no multiple of either image's pixel count)

// h, the held form of k, as the masks of a wide input
static lpf_wide_input wide_input(const Held &h, const Rle &k)
{
    lpf_wide_input wi;
    memset(&wi, 0, sizeof wi);
    wi.masks = h.in; wi.M = k.M; wi.f32 = LPF_MASKS_RLE; wi.erode_iters = k.erode;
    wi.rects = (const int32_t *)16; wi.binarize = 77;    // neither is read in this form
    return wi;
}

// drive_common.h's, with this driver's image as the default
static Rle simple(int F, int M, int runs_per_mask, int length = 3, int hw = HW);
static bool in_force(lpf_ctx *c, int F, int hw = HW);

static std::vector<float> g_pts(4 * (size_t)NPTS * 3, 1.0f);
static int64_t g_off[4] = {0, NPTS, 2 * NPTS, 3 * NPTS};

// lpf_run_wide with k as its masks; the arrays are gone when it returns
static int run_wide(lpf_ctx *c, const Rle &k, int F)
{
    Dev D;
    lpf_wide_outputs o;
    wide_outputs(D, o, F, k.M > 0 && k.M <= LPF_MAX_MASKS_WIDE ? k.M : 1, NPTS);
    Held h(k);
    const lpf_wide_input wi = wide_input(h, k);
    const int rc = lpf_run_wide(c, g_pts.data(), g_off, F, 0, &wi, &o);
    h.release();
    if (rc == LPF_OK && k.M > 0) fprintf(stderr, "dense-bytes %lld\n", (long long)F * k.M * HW);
    return rc;
}

static void camera(lpf_cam_input &I, int w, int h)
{
    memset(&I, 0, sizeof I);
    memcpy(I.T_velo_to_rect, T16, sizeof T16);
    memcpy(I.K, K9, sizeof K9);
    I.W = w; I.H = h; I.depth_min_excl = 0; I.depth_max_excl = 50;
}

// a pass over two cameras (37 x 23 with k0, 30 x 20 with k1; NULL: that camera has no masks): lpf_run_cams_wide or lpf_run_cams
static int run_cams(lpf_ctx *c, bool wide, const Rle *k0, const Rle *k1, int F)
{
    Dev D;
    const Rle *ks[2] = {k0, k1};
    lpf_cam_input cams[2];
    camera(cams[0], W, H);
    camera(cams[1], W1, H1);
    std::vector<Held> held;
    held.reserve(2);
    lpf_wide_outputs ow[2];
    lpf_outputs on[2];
    const int limit = wide ? LPF_MAX_MASKS_WIDE : LPF_MAX_MASKS;
    for (int k = 0; k < 2; ++k) {
        const int M = ks[k] && ks[k]->M > 0 && ks[k]->M <= limit ? ks[k]->M : 1;
        wide_outputs(D, ow[k], F, M, NPTS);
        narrow_outputs(D, on[k], F, M, NPTS);
        if (!ks[k]) continue;
        held.emplace_back(*ks[k]);
        cams[k].masks = wide_input(held.back(), *ks[k]);
    }
    const int rc = wide ? lpf_run_cams_wide(c, g_pts.data(), g_off, F, 0, cams, 2, ow) : lpf_run_cams(c, g_pts.data(), g_off, F, 0, cams, 2, on);
    for (Held &h : held) h.release();
    if (rc == LPF_OK)
        for (int k = 0; k < 2; ++k)
            if (ks[k] && ks[k]->M > 0) fprintf(stderr, "dense-bytes %lld\n", (long long)F * ks[k]->M * (k ? HW1 : HW));
    return rc;
}

static void refusals(lpf_ctx *c)
{
    // the narrow state every call below must leave alone
    {
        const Rle n = simple(2, 3, 2);
        Held h(n);
        CHECK(lpf_set_masks_rle(c, h.in) == LPF_OK);
        h.release();
        CHECK(in_force(c, 2));
    }
    CHECK(run_wide(c, simple(1, 5, 2), 1) == LPF_OK);        // (the passes' buffers exist; these are fine as they are)
    for (int wide = 0; wide < 2; ++wide) {
        const Rle a = simple(1, 5, 2), b = simple(1, 5, 2, 3, HW1);
        CHECK(run_cams(c, wide, &a, &b, 1) == LPF_OK);
    }
    const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
    char want[512];
    Rle k;

    // ---- lpf_run_wide: the struct must describe the call
    k = simple(2, 5, 2);
    CHECK(run_wide(c, k, 1) == LPF_ERR_ARG && err_is("run_wide: the run-length masks say F=2 M=5 erode_iters=0, the call has F=1 M=5 erode_iters=0"));
    {
        k = simple(1, 5, 2);
        Held h(k);
        lpf_wide_input wi = wide_input(h, k);
        Dev D;
        lpf_wide_outputs o;
        wide_outputs(D, o, 1, 6, NPTS);
        wi.M = 6;
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 1, 0, &wi, &o) == LPF_ERR_ARG &&
              err_is("run_wide: the run-length masks say F=1 M=5 erode_iters=0, the call has F=1 M=6 erode_iters=0"));
        wi.M = 5; wi.erode_iters = 2;
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 1, 0, &wi, &o) == LPF_ERR_ARG &&
              err_is("run_wide: the run-length masks say F=1 M=5 erode_iters=0, the call has F=1 M=5 erode_iters=2"));
        wi.erode_iters = 0; wi.on_device = 1;
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 1, 0, &wi, &o) == LPF_ERR_ARG &&
              err_is("run_wide: f32=LPF_MASKS_RLE with on_device=1: run-length masks are host memory (on_device 0)"));
        wi.on_device = 0; wi.f32 = 3;
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 1, 0, &wi, &o) == LPF_ERR_ARG &&
              err_is("run_wide: f32=3 (LPF_MASKS_U8 = 0, LPF_MASKS_F32 = 1 or LPF_MASKS_RLE = 2)"));
        wi.f32 = -1;
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 1, 0, &wi, &o) == LPF_ERR_ARG &&
              err_is("run_wide: f32=-1 (LPF_MASKS_U8 = 0, LPF_MASKS_F32 = 1 or LPF_MASKS_RLE = 2)"));
        wi.f32 = LPF_MASKS_RLE; wi.M = LPF_MAX_MASKS_WIDE + 1;       // (refused before the struct is looked at)
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 1, 0, &wi, &o) == LPF_ERR_ARG &&
              err_is("run_wide: M=257 masks per frame, lpf_run_wide takes 0 .. LPF_MAX_MASKS_WIDE = 256"));
        h.release();
    }
    // ---- ... and lpf_set_masks_rle's rules, with the call's prefix
    k = simple(1, 5, 2); k.reserved = 7;
    CHECK(run_wide(c, k, 1) == LPF_ERR_ARG && err_is("run_wide: F=1 M=5 erode_iters=0 reserved=7"));
    k = simple(1, 5, 2); k.off[0] = 1;
    CHECK(run_wide(c, k, 1) == LPF_ERR_ARG && err_is("run_wide: run_off[0]=1 (must be 0)"));
    k = simple(2, 3, 2); k.off[5] = 7;                       // 0 2 4 6 8 7 12: decreases at k = 4 -> frame 1 mask 1
    CHECK(run_wide(c, k, 2) == LPF_ERR_ARG && err_is("run_wide: run_off decreases at frame 1 mask 1 (7 after 8)"));
    k = simple(1, 2, 1); k.off.clear();
    CHECK(run_wide(c, k, 1) == LPF_ERR_ARG && err_is("run_wide: run_off=NULL with F=1 M=2"));
    k = simple(1, 2, 1); k.runs.clear();
    CHECK(run_wide(c, k, 1) == LPF_ERR_ARG && err_is("run_wide: runs=NULL with 2 runs"));
    struct Bad { int32_t start, length; } bad[] = {{-1, 3}, {5, -1}, {HW - 2, 3}, {HW, 1}, {INT32_MAX, INT32_MAX}, {0, HW + 1}, {INT32_MIN, 0}};
    for (const Bad &b : bad) {
        k = simple(2, 40, 2);                                // run 1 of frame 1, mask 33: global run 2 * (40 + 33) + 1
        const int g = 2 * (40 + 33) + 1;
        k.runs[2 * g] = b.start; k.runs[2 * g + 1] = b.length;
        snprintf(want, sizeof want, "run_wide: frame 1 mask 33 run 1: start=%d length=%d (0 <= start, 0 <= length, start + length <= W*H = %d)",
                 b.start, b.length, HW);
        CHECK(run_wide(c, k, 2) == LPF_ERR_ARG && err_is(want));
    }

    // ---- the camera passes: each camera against its own image
    for (int wide = 0; wide < 2; ++wide) {
        const char *who = wide ? "run_cams_wide" : "run_cams";
        Rle a = simple(1, 5, 2), b = simple(1, 5, 2, 3, HW1);
        a.runs[0] = HW1 - 2; b.runs[0] = HW1 - 2;            // one pixel past camera 1's image, well inside camera 0's
        snprintf(want, sizeof want, "%s: camera 1: frame 0 mask 0 run 0: start=%d length=3 (0 <= start, 0 <= length, start + length <= W*H = %d)",
                 who, HW1 - 2, HW1);
        CHECK(run_cams(c, wide, &a, &b, 1) == LPF_ERR_ARG && err_is(want));
        b = simple(1, 5, 2, 3, HW1);
        a.runs[0] = HW - 2;                                  // ... and camera 0's own limit
        snprintf(want, sizeof want, "%s: camera 0: frame 0 mask 0 run 0: start=%d length=3 (0 <= start, 0 <= length, start + length <= W*H = %d)",
                 who, HW - 2, HW);
        CHECK(run_cams(c, wide, &a, &b, 1) == LPF_ERR_ARG && err_is(want));
        a = simple(1, 5, 2); b = simple(2, 5, 2, 3, HW1);
        snprintf(want, sizeof want, "%s: camera 1: the run-length masks say F=2 M=5 erode_iters=0, the call has F=1 M=5 erode_iters=0", who);
        CHECK(run_cams(c, wide, &a, &b, 1) == LPF_ERR_ARG && err_is(want));
        b = simple(1, 5, 2, 3, HW1); b.reserved = 1;
        snprintf(want, sizeof want, "%s: camera 1: F=1 M=5 erode_iters=0 reserved=1", who);
        CHECK(run_cams(c, wide, &a, &b, 1) == LPF_ERR_ARG && err_is(want));
        {
            Held h(a);
            lpf_cam_input cam;
            camera(cam, W, H);
            cam.masks = wide_input(h, a);
            Dev D;
            lpf_wide_outputs ow;
            lpf_outputs on;
            wide_outputs(D, ow, 1, 5, NPTS);
            narrow_outputs(D, on, 1, 5, NPTS);
            auto call = [&] { return wide ? lpf_run_cams_wide(c, g_pts.data(), g_off, 1, 0, &cam, 1, &ow) : lpf_run_cams(c, g_pts.data(), g_off, 1, 0, &cam, 1, &on); };
            cam.masks.on_device = 2;
            snprintf(want, sizeof want, "%s: camera 0: f32=LPF_MASKS_RLE with on_device=2: run-length masks are host memory (on_device 0)", who);
            CHECK(call() == LPF_ERR_ARG && err_is(want));
            cam.masks.on_device = 0; cam.masks.f32 = 3;
            snprintf(want, sizeof want, "%s: camera 0: f32=3 (LPF_MASKS_U8 = 0, LPF_MASKS_F32 = 1 or LPF_MASKS_RLE = 2)", who);
            CHECK(call() == LPF_ERR_ARG && err_is(want));
            cam.masks.f32 = LPF_MASKS_RLE; cam.masks.M = 6;
            snprintf(want, sizeof want, "%s: camera 0: the run-length masks say F=1 M=5 erode_iters=0, the call has F=1 M=6 erode_iters=0", who);
            CHECK(call() == LPF_ERR_ARG && err_is(want));
            h.release();
        }
    }
    k = simple(1, LPF_MAX_MASKS + 1, 1);
    CHECK(run_cams(c, false, &k, nullptr, 1) == LPF_ERR_ARG &&
          err_is("run_cams: camera 0 has M=33 masks per frame, a pass takes 0 .. LPF_MAX_MASKS = 32 per camera (more: lpf_run_wide for that camera)"));
    CHECK(fake_hip_launches() == l0 && fake_hip_copies() == c0);

    // ---- the calls that keep their dense masks refuse the form by name, before `masks` is read (here it points nowhere)
    {
        lpf_wide_input wi;
        memset(&wi, 0, sizeof wi);
        wi.masks = (const void *)8; wi.M = 5; wi.f32 = LPF_MASKS_RLE;
        Dev D;
        lpf_depth_maps_outputs dm;
        memset(&dm, 0, sizeof dm);
        dm.cap = 50; dm.pix = D.get<int64_t>(50); dm.depth = D.get<double>(50); dm.point_idx = D.get<int64_t>(50); dm.car_off = D.get<int64_t>(6);
        dm.need = D.get<int64_t>(1); dm.overflow = D.get<int32_t>(1);
        CHECK(lpf_depth_maps(c, g_pts.data(), g_off, 1, 0, &wi, &dm) == LPF_ERR_ARG &&
              err_is("depth_maps: f32=LPF_MASKS_RLE: lpf_depth_maps takes dense masks only (run-length masks: lpf_run_wide, lpf_run_cams, lpf_run_cams_wide)"));
        wi.f32 = 3;
        CHECK(lpf_depth_maps(c, g_pts.data(), g_off, 1, 0, &wi, &dm) == LPF_ERR_ARG &&
              err_is("depth_maps: f32=3 (LPF_MASKS_U8 = 0, LPF_MASKS_F32 = 1 or LPF_MASKS_RLE = 2)"));
        lpf_first_match_input fi;
        memset(&fi, 0, sizeof fi);
        fi.masks = (const void *)8; fi.M = 5; fi.mh = H; fi.mw = W; fi.f32 = LPF_MASKS_RLE;
        lpf_first_match_outputs fo;
        memset(&fo, 0, sizeof fo);
        fo.n_car = D.get<int64_t>(1); fo.n_bg = D.get<int64_t>(1);
        CHECK(lpf_first_match(c, g_pts.data(), g_off, 1, 0, &fi, &fo) == LPF_ERR_ARG &&
              err_is("first_match: f32=2 (LPF_MASKS_U8 = 0 or LPF_MASKS_F32 = 1: lpf_first_match takes dense masks only)"));
    }
    // nothing was queued by any refusal, and the narrow masks are still in force
    CHECK(fake_hip_launches() == l0 && fake_hip_copies() == c0);
    CHECK(in_force(c, 2));
    // the limits themselves are fine: the whole image, its last pixel, an empty run at the very end
    k = simple(1, 33, 3);
    const int32_t edge[6] = {0, HW, HW - 1, 1, HW, 0};
    memcpy(k.runs.data() + 6 * 32, edge, sizeof edge);       // mask 32: bit 0 of word 1
    CHECK(run_wide(c, k, 1) == LPF_OK && in_force(c, 2));
}

static long long launches_of(lpf_ctx *c, const Rle &k, int F)
{
    const long long l0 = fake_hip_launches();
    CHECK(run_wide(c, k, F) == LPF_OK);
    return fake_hip_launches() - l0;
}

static void no_decode(lpf_ctx *c)
{
    // masks without runs, and runs that are all empty, whatever erode_iters asks for: one launch fewer than the same masks with runs
    Rle k = simple(2, 40, 2);
    const long long with_runs = launches_of(c, k, 2);
    k = simple(2, 40, 0);
    const long long none = launches_of(c, k, 2);
    CHECK(with_runs - none == 1);                            // the decode
    k = simple(2, 40, 0); k.erode = 2;
    CHECK(launches_of(c, k, 2) == none);
    k = simple(2, 40, 2, 0); k.erode = 1;
    CHECK(launches_of(c, k, 2) == none);
    // erosion: every iteration is a launch of its own (none fused); the k x k element; the 1 x 1 element is the identity
    k = simple(2, 40, 2); k.erode = 2;
    CHECK(launches_of(c, k, 2) == with_runs + 2);
    CHECK(lpf_set_erosion_element(c, 5) == LPF_OK);
    CHECK(launches_of(c, k, 2) == with_runs + 2);
    CHECK(lpf_set_erosion_element(c, 1) == LPF_OK);
    CHECK(launches_of(c, k, 2) == with_runs);
    CHECK(lpf_set_erosion_element(c, 3) == LPF_OK);
    // M = 0: no masks -- with the struct (run_off has its one entry, or is not given), and without one
    k = Rle(); k.F = 2; k.M = 0; k.off = {0};
    const long long m0 = launches_of(c, k, 2);
    k.off.clear();
    CHECK(launches_of(c, k, 2) == m0);
    {
        lpf_wide_input wi;
        memset(&wi, 0, sizeof wi);
        wi.f32 = LPF_MASKS_RLE;
        Dev D;
        lpf_wide_outputs o;
        wide_outputs(D, o, 2, 1, NPTS);
        const long long l0 = fake_hip_launches();
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 2, 0, &wi, &o) == LPF_OK && fake_hip_launches() - l0 == m0);
        wi.f32 = LPF_MASKS_U8;                               // ... as many launches as dense M = 0
        const long long l1 = fake_hip_launches();
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 2, 0, &wi, &o) == LPF_OK && fake_hip_launches() - l1 == m0);
    }
    CHECK(m0 < none);
    // the camera passes: a camera without runs costs no decode
    for (int wide = 0; wide < 2; ++wide) {
        Rle a = simple(2, 9, 2), b = simple(2, 20, 2, 3, HW1), e = simple(2, 20, 0, 3, HW1);
        long long l0 = fake_hip_launches();
        CHECK(run_cams(c, wide, &a, &b, 2) == LPF_OK);
        const long long both = fake_hip_launches() - l0;
        l0 = fake_hip_launches();
        CHECK(run_cams(c, wide, &a, &e, 2) == LPF_OK);
        CHECK(both - (fake_hip_launches() - l0) == 1);
        a.erode = 1; b.erode = 2;
        l0 = fake_hip_launches();
        CHECK(run_cams(c, wide, &a, &b, 2) == LPF_OK);
        CHECK(fake_hip_launches() - l0 == both + 3);
    }
}

static void sizes(lpf_ctx *c)
{
    // M = 256, F = 3: shuffled order, overlaps and repeats, ragged with empty masks; eroded
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
    CHECK(run_wide(c, big, 3) == LPF_OK);
    big.erode = 2;
    CHECK(run_wide(c, big, 3) == LPF_OK);
    // two run-length cameras in one pass, of different sizes and widths
    {
        Rle a = simple(3, 40, 5), b = simple(3, 5, 4, 7, HW1);
        CHECK(run_cams(c, true, &a, &b, 3) == LPF_OK);
        CHECK(run_cams(c, true, &a, nullptr, 3) == LPF_OK);          // (the other camera has no masks)
        Rle n0 = simple(3, 9, 5), n1 = simple(3, 20, 4, 7, HW1);
        CHECK(run_cams(c, false, &n0, &n1, 3) == LPF_OK);
        Rle s0 = simple(3, 8, 5), s1 = simple(3, 3, 4, 7, HW1);      // all narrow: one-byte label elements
        s1.erode = 1;
        CHECK(run_cams(c, false, &s0, &s1, 3) == LPF_OK);
        CHECK(run_cams(c, false, nullptr, &s1, 3) == LPF_OK);
    }
    // growing then shrinking calls on the same context
    for (int F : {1, 3, 2, 1})
        for (int M : {1, 33, 256, 40, 5}) {
            Rle k = simple(F, M, F + M % 7, 1 + M % 9);
            k.erode = M % 3;
            CHECK(run_wide(c, k, F) == LPF_OK);
            Rle k1 = simple(F, M, 2 + M % 5, 1 + M % 9, HW1);
            CHECK(run_cams(c, true, &k, &k1, F) == LPF_OK);
        }
    // one run that is a whole larger image, as mask 32
    CHECK(lpf_set_camera(c, T16, K9, 1408, 376, 0, 50) == LPF_OK);
    {
        Rle full;
        full.F = 1; full.M = 33; full.runs = {0, 1408 * 376}; full.off.assign(34, 0); full.off[33] = 1;
        Dev D;
        lpf_wide_outputs o;
        wide_outputs(D, o, 1, 33, NPTS);
        Held h(full);
        const lpf_wide_input wi = wide_input(h, full);
        const long long l0 = fake_hip_launches();
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 1, 0, &wi, &o) == LPF_OK);
        h.release();
        CHECK(fake_hip_launches() > l0);
    }
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
}

// a pipelined context with a narrow run owed: the wide call launches what is owed and runs in order; the narrow masks stay in force
static void pipelined(lpf_ctx *c)
{
    for (int mode : {2, 4, 0}) {
        CHECK(lpf_set_pipelined(c, mode) == LPF_OK);
        Dev D;
        lpf_outputs o;
        narrow_outputs(D, o, 1, 5, NPTS);
        for (int it = 0; it < 3; ++it) {
            const Rle n = simple(1, 5 + 6 * it, 3);
            Held h(n);
            CHECK(lpf_set_masks_rle(c, h.in) == LPF_OK);
            h.release();
            CHECK(lpf_run_batch(c, g_pts.data(), g_off, 1, 0, &o) == LPF_OK);        // owed, in modes 2 / 4
            Rle k = simple(1, 40 + it, 3);
            k.erode = it;
            CHECK(run_wide(c, k, 1) == LPF_OK);
            Rle a = simple(1, 9, 2), b = simple(1, 20, 2, 3, HW1);
            CHECK(run_cams(c, it & 1, &a, &b, 1) == LPF_OK);
        }
        CHECK(lpf_sync(c) == LPF_OK);
    }
    CHECK(in_force(c, 1));
}

int main()
{
    lpf_ctx *c = drive_begin();
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    refusals(c);
    no_decode(c);
    sizes(c);
    pipelined(c);
    lpf_destroy(c);
    return drive_finish("drive_rle_wide", false);
}
