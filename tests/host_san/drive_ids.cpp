// drive_ids.cpp -- drives the HOST side of instance-ID maps (lpf_set_masks_ids, lpf_run_wide_ids; lpf_api.hip compiled
// --offload-host-only against fake_hip.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer: every refusal of both calls with its
// message and nothing queued, the state errors (no camera, inside a capture), F = 0 and M = 0 without a decode launch, the launches of
// calls with erosion, growing then shrinking calls with both ID types and maps in host and in "device" memory (a map whose base is
// aligned to its element only among them), the 1408 x 376 image, both pipelined modes with a narrow run owed, and -- as a section of its
// own, `drive_ids mixed` -- lpf_run_wide with dense masks after lpf_run_wide_ids on the same context.  sel, host ids AND the lpf_id_masks
// struct live in exactly-sized heap blocks that are scribbled over and freed as soon as the call has returned, so a read past either
// end, or after the call, is an error here.  `drive_ids ids` runs everything but the mixed section: ID maps only, so that
// tests/test_host_sanitized_ids.py can say from the FAKE_HIP_TRACE file which kernels the form launches and what it copies.  Each
// successful call with M > 4 prints what its dense twin would have copied ("dense-bytes N") and the bytes of the image or planes it
// writes ("written-bytes N": no memset of that size may appear).  Results are checked on the GPU by tests/test_gpu_ids.py.
#include "drive_common.h"
#include <climits>

static int W = 37, H = 23, HW = W * H;                       // the camera in force (camera())
static bool in_force(lpf_ctx *c, int F, int hw = HW);       // (drive_common.h's; the default is read at each call)
static const int NPTS = 1001;

static void camera(lpf_ctx *c, int w, int h)
{
    CHECK(lpf_set_camera(c, T16, K9, w, h, 0, 50) == LPF_OK);
    W = w; H = h; HW = w * h;
}

// one set of ID maps as a caller describes it
struct Ids {
    int F = 1, M = 1, id_bytes = 2, erode = 0, on_device = 0, reserved = 0;
    bool no_ids = false, no_sel = false, misalign = false;   // NULL pointers; a device map one element behind its allocation's start
};

// ... and as it is handed over: sel, host ids and the struct in exactly-sized heap blocks; release(): scribble and free
struct HeldIds {
    void *ids = nullptr, *dev = nullptr;
    int32_t *sel = nullptr;
    lpf_id_masks *in = nullptr;
    size_t nb = 0, ns = 0;
    explicit HeldIds(const Ids &k)
    {
        const int bytes = k.id_bytes == 4 ? 4 : 2;
        const long long F = k.F > 0 ? k.F : 0, M = k.M > 0 ? k.M : 0;
        nb = (size_t)F * HW * bytes;
        ns = F * M < (1 << 20) ? (size_t)(F * M) : 0;       // (a table refused for its size is never read)
        if (nb && !k.no_ids) {
            if (k.on_device) {
                if (hipMalloc(&dev, nb + 16) != 0) abort();
                ids = (char *)dev + (k.misalign ? bytes : 0);
            } else {
                ids = malloc(nb);
            }
            for (size_t i = 0; i < nb / bytes; ++i) {
                if (bytes == 2) ((uint16_t *)ids)[i] = (uint16_t)(i * 7 % 50); else ((int32_t *)ids)[i] = (int32_t)(i * 7 % 50) - 3;
            }
        }
        if (ns && !k.no_sel) {
            sel = (int32_t *)malloc(ns * sizeof(int32_t));
            for (size_t i = 0; i < ns; ++i) sel[i] = i % 5 == 4 ? LPF_ID_NONE : (int32_t)(i % 60) - 3;
        }
        in = (lpf_id_masks *)malloc(sizeof(lpf_id_masks));
        memset(in, 0, sizeof *in);
        in->ids = ids; in->sel = sel; in->F = k.F; in->M = k.M; in->id_bytes = k.id_bytes; in->erode_iters = k.erode;
        in->on_device = k.on_device; in->reserved = k.reserved;
    }
    void release()                                           // the library has its copies: scribble, then free
    {
        if (sel) memset(sel, 0xEE, ns * sizeof(int32_t));
        if (ids && !dev) memset(ids, 0xEE, nb);
        memset(in, 0xEE, sizeof *in);
        free(sel); free(in);
        if (!dev) free(ids);
        sel = nullptr; in = nullptr; ids = nullptr;
    }
    void release_device(lpf_ctx *c)                          // a lent map: after the work that reads it
    {
        if (!dev) return;
        CHECK(lpf_sync(c) == LPF_OK);
        hipFree(dev);
        dev = nullptr;
    }
};

static Ids ids_of(int F, int M, int id_bytes = 2, int on_device = 0, int erode = 0)
{
    Ids k;
    k.F = F; k.M = M; k.id_bytes = id_bytes; k.on_device = on_device; k.erode = erode;
    return k;
}

static void said(const Ids &k, int lw_or_lb_bytes)
{
    if (k.M <= 4) return;
    fprintf(stderr, "dense-bytes %lld\n", (long long)k.F * k.M * HW);
    fprintf(stderr, "written-bytes %lld\n", (long long)k.F * HW * lw_or_lb_bytes);
}

static int set_ids(lpf_ctx *c, const Ids &k)
{
    HeldIds h(k);
    const int rc = lpf_set_masks_ids(c, h.in);
    h.release();
    h.release_device(c);
    if (rc == LPF_OK && k.F > 0) said(k, k.M <= 8 ? 1 : k.M <= 16 ? 2 : 4);
    return rc;
}

static std::vector<float> g_pts(4 * (size_t)NPTS * 8, 1.0f);
static int64_t g_off[9] = {0, NPTS, 2 * NPTS, 3 * NPTS, 4 * NPTS, 5 * NPTS, 6 * NPTS, 7 * NPTS, 8 * NPTS};

// lpf_run_wide_ids for F frames with k as its maps; the arrays are gone when it returns
static int run_ids(lpf_ctx *c, const Ids &k, int F)
{
    Dev D;
    lpf_wide_outputs o;
    wide_outputs(D, o, F > 0 ? F : 1, k.M > 0 && k.M <= LPF_MAX_MASKS_WIDE ? k.M : 1, NPTS);
    HeldIds h(k);
    const int rc = lpf_run_wide_ids(c, g_pts.data(), g_off, F, 0, h.in, &o);
    h.release();
    h.release_device(c);
    if (rc == LPF_OK) said(k, 4 * ((k.M + 31) / 32));
    return rc;
}

static void state_errors(lpf_ctx *c)
{
    const Ids k = ids_of(1, 5), w = ids_of(1, 40);
    lpf_id_masks in;
    memset(&in, 0, sizeof in);
    CHECK(lpf_set_masks_ids(nullptr, &in) == LPF_ERR_ARG);
    CHECK(lpf_run_wide_ids(nullptr, nullptr, nullptr, 1, 0, &in, nullptr) == LPF_ERR_ARG);
    CHECK(set_ids(c, k) == LPF_ERR_STATE && err_is("lpf_set_camera must be called before masks (W, H)"));
    CHECK(run_ids(c, w, 1) == LPF_ERR_STATE && err_is("lpf_set_camera has not been called"));
    camera(c, 37, 23);
    CHECK(set_ids(c, k) == LPF_OK && run_ids(c, w, 1) == LPF_OK);    // (buffers exist: a capture could take the launches)
    for (int which = 0; which < 2; ++which) {
        CHECK(lpf_graph_begin(c) == LPF_OK);
        const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
        if (which == 0) CHECK(set_ids(c, k) == LPF_ERR_STATE && err_has("lpf_set_masks_ids cannot be captured into a graph"));
        else CHECK(run_ids(c, w, 1) == LPF_ERR_STATE && err_has("lpf_run_wide_ids cannot be captured into a graph"));
        CHECK(fake_hip_launches() == l0 && fake_hip_copies() == c0);
        lpf_graph *g = nullptr;
        (void)lpf_graph_end(c, &g);                          // (the refusal abandoned the capture, as every error inside one does)
        if (g) lpf_graph_destroy(g);
    }
    CHECK(set_ids(c, k) == LPF_OK && in_force(c, 1));
}

static void refusals(lpf_ctx *c)
{
    CHECK(set_ids(c, ids_of(2, 3)) == LPF_OK && in_force(c, 2));     // what every refusal below must leave in force
    const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
    char want[512];
    Ids k;
    // lpf_set_masks_ids
    CHECK(lpf_set_masks_ids(c, nullptr) == LPF_ERR_ARG && err_is("lpf_set_masks_ids: in=NULL"));
    k = ids_of(-1, 2);
    CHECK(set_ids(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_ids: F=-1 (must be >= 0)"));
    k = ids_of(1, -1);
    CHECK(set_ids(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_ids: M=-1 (must be >= 0)"));
    k = ids_of(1, 2); k.erode = -2;
    CHECK(set_ids(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_ids: erode_iters=-2 (must be >= 0)"));
    for (int bytes : {0, 1, 3, 8, -2}) {
        k = ids_of(1, 2); k.id_bytes = bytes;
        snprintf(want, sizeof want, "lpf_set_masks_ids: id_bytes=%d (2: uint16 IDs, 4: int32 IDs)", bytes);
        CHECK(set_ids(c, k) == LPF_ERR_ARG && err_is(want));
    }
    for (int where : {2, -1}) {
        k = ids_of(1, 2);
        HeldIds h(k);
        h.in->on_device = where;
        snprintf(want, sizeof want, "lpf_set_masks_ids: on_device=%d (0: ids in host memory, 1: device memory)", where);
        CHECK(lpf_set_masks_ids(c, h.in) == LPF_ERR_ARG && err_is(want));
        h.release();
    }
    k = ids_of(1, 2); k.reserved = 7;
    CHECK(set_ids(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_ids: reserved=7 (must be 0)"));
    k = ids_of(1, LPF_MAX_MASKS + 1);                        // (refused before the arrays are looked at)
    snprintf(want, sizeof want, "set_masks: M=%d masks per frame, a run takes at most LPF_MAX_MASKS = %d (one bit each in label_bits): run the frame "
                                "once per group of %d masks -- everything per point is the same in every pass (pipeline.run_frames does so)",
             LPF_MAX_MASKS + 1, LPF_MAX_MASKS, LPF_MAX_MASKS);
    CHECK(set_ids(c, k) == LPF_ERR_ARG && err_is(want));
    {                                                        // ... the message lpf_set_masks_u8 gives
        uint8_t one = 0;
        CHECK(lpf_set_masks_u8(c, &one, 1, LPF_MAX_MASKS + 1, 0, 0) == LPF_ERR_ARG && err_is(want));
    }
    k = ids_of(1, 2); k.no_ids = true;
    CHECK(set_ids(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_ids: ids=NULL with F=1"));
    k = ids_of(1, 0); k.no_ids = true;                       // (also without masks: the map is what F frames are)
    CHECK(set_ids(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_ids: ids=NULL with F=1"));
    k = ids_of(2, 3); k.no_sel = true;
    CHECK(set_ids(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_ids: sel=NULL with F=2 M=3"));
    {                                                        // F * M above 2^31 - 1: refused before either array is looked at
        lpf_id_masks in;
        memset(&in, 0, sizeof in);
        in.ids = &in; in.sel = (const int32_t *)&in; in.F = INT32_MAX; in.M = 2; in.id_bytes = 2;
        CHECK(lpf_set_masks_ids(c, &in) == LPF_ERR_ARG && err_is("lpf_set_masks_ids: F * M = 4294967294 table entries (at most 2^31 - 1 in one call)"));
    }
    // lpf_run_wide_ids
    Dev D;
    lpf_wide_outputs o;
    wide_outputs(D, o, 2, 40, NPTS);
    CHECK(lpf_run_wide_ids(c, g_pts.data(), g_off, 2, 0, nullptr, &o) == LPF_ERR_ARG && err_is("run_wide_ids: in=NULL"));
    k = ids_of(2, LPF_MAX_MASKS_WIDE + 1);
    CHECK(run_ids(c, k, 2) == LPF_ERR_ARG && err_is("run_wide_ids: M=257 masks per frame, lpf_run_wide_ids takes 0 .. LPF_MAX_MASKS_WIDE = 256"));
    k = ids_of(2, -1);
    CHECK(run_ids(c, k, 2) == LPF_ERR_ARG && err_is("run_wide_ids: M=-1 (must be >= 0)"));
    k = ids_of(-2, 40);
    CHECK(run_ids(c, k, 2) == LPF_ERR_ARG && err_is("run_wide_ids: F=-2 (must be >= 0)"));
    k = ids_of(2, 40); k.erode = -1;
    CHECK(run_ids(c, k, 2) == LPF_ERR_ARG && err_is("run_wide_ids: erode_iters=-1 (must be >= 0)"));
    k = ids_of(2, 40); k.id_bytes = 3;
    CHECK(run_ids(c, k, 2) == LPF_ERR_ARG && err_is("run_wide_ids: id_bytes=3 (2: uint16 IDs, 4: int32 IDs)"));
    k = ids_of(2, 40); k.reserved = -1;
    CHECK(run_ids(c, k, 2) == LPF_ERR_ARG && err_is("run_wide_ids: reserved=-1 (must be 0)"));
    k = ids_of(2, 40); k.no_ids = true;
    CHECK(run_ids(c, k, 2) == LPF_ERR_ARG && err_is("run_wide_ids: ids=NULL with F=2"));
    k = ids_of(2, 40); k.no_sel = true;
    CHECK(run_ids(c, k, 2) == LPF_ERR_ARG && err_is("run_wide_ids: sel=NULL with F=2 M=40"));
    {
        k = ids_of(2, 40);
        HeldIds h(k);
        h.in->on_device = 2;
        CHECK(lpf_run_wide_ids(c, g_pts.data(), g_off, 2, 0, h.in, &o) == LPF_ERR_ARG && err_is("run_wide_ids: on_device=2 (0: ids in host memory, 1: device memory)"));
        h.release();
    }
    k = ids_of(3, 40);
    CHECK(run_ids(c, k, 2) == LPF_ERR_ARG && err_is("run_wide_ids: the ID maps say F=3, the call has F=2"));
    k = ids_of(0, 40);                                       // lpf_run_wide's own: no frames
    CHECK(run_ids(c, k, 0) == LPF_ERR_ARG && err_has("run_wide_ids: in=") && err_has("F=0"));
    {                                                        // ... no outputs, no frame_off, a frame_off that does not start at 0
        k = ids_of(2, 40);
        HeldIds h(k);
        CHECK(lpf_run_wide_ids(c, g_pts.data(), g_off, 2, 0, h.in, nullptr) == LPF_ERR_ARG && err_has("run_wide_ids: in="));
        CHECK(lpf_run_wide_ids(c, g_pts.data(), nullptr, 2, 0, h.in, &o) == LPF_ERR_ARG && err_has("run_wide_ids: in="));
        CHECK(lpf_run_wide_ids(c, g_pts.data(), g_off + 1, 2, 0, h.in, &o) == LPF_ERR_ARG && err_is("run_wide_ids: frame_off[0] must be 0"));
        h.release();
    }
    // nothing was queued by any of them, and the masks set before are still in force
    CHECK(fake_hip_launches() == l0 && fake_hip_copies() == c0);
    CHECK(in_force(c, 2));
    // lpf_wide_input.f32 has no fourth value: the refusal and its message stay
    {
        lpf_wide_input wi;
        memset(&wi, 0, sizeof wi);
        wi.masks = &wi; wi.M = 3; wi.f32 = 3;
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 2, 0, &wi, &o) == LPF_ERR_ARG && err_is("run_wide: f32=3 (LPF_MASKS_U8 = 0, LPF_MASKS_F32 = 1 or LPF_MASKS_RLE = 2)"));
    }
}

static void no_decode(lpf_ctx *c)
{
    // F = 0: as lpf_set_masks_rle with F = 0 -- no masks in force, nothing queued (neither pointer is needed)
    long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
    Ids k = ids_of(0, 5);
    CHECK(set_ids(c, k) == LPF_OK && fake_hip_launches() == l0 && fake_hip_copies() == c0);
    CHECK(in_force(c, 0));
    // M = 0: a zeroed image in force, no decode, no copy (sel is not needed; F = 5 is this call's alone: its memset is recognisable)
    l0 = fake_hip_launches(); c0 = fake_hip_copies();
    k = ids_of(5, 0); k.no_sel = true;
    CHECK(set_ids(c, k) == LPF_OK && fake_hip_launches() == l0 && fake_hip_copies() == c0);
    CHECK(in_force(c, 5));
    // the wide call without masks launches what lpf_run_wide launches without masks
    l0 = fake_hip_launches();
    k = ids_of(2, 0); k.no_sel = true;
    CHECK(run_ids(c, k, 2) == LPF_OK);
    const long long none = fake_hip_launches() - l0;
    {
        Dev D;
        lpf_wide_outputs o;
        wide_outputs(D, o, 2, 1, NPTS);
        lpf_wide_input wi;
        memset(&wi, 0, sizeof wi);
        l0 = fake_hip_launches();
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 2, 0, &wi, &o) == LPF_OK && fake_hip_launches() - l0 == none);
    }
    CHECK(in_force(c, 5));                                   // (the narrow state is untouched by the wide calls)
}

static void launches(lpf_ctx *c)
{
    long long l0 = fake_hip_launches();
    Ids k = ids_of(2, 9);
    CHECK(set_ids(c, k) == LPF_OK && fake_hip_launches() - l0 == 1);             // the decode
    l0 = fake_hip_launches();
    k.erode = 2;
    CHECK(set_ids(c, k) == LPF_OK && fake_hip_launches() - l0 == 3);             // decode + 2 erosions (none of them fused)
    CHECK(lpf_set_erosion_element(c, 5) == LPF_OK);
    l0 = fake_hip_launches();
    CHECK(set_ids(c, k) == LPF_OK && fake_hip_launches() - l0 == 3);             // ... with the k x k element
    CHECK(lpf_set_erosion_element(c, 1) == LPF_OK);                              // the identity
    l0 = fake_hip_launches();
    CHECK(set_ids(c, k) == LPF_OK && fake_hip_launches() - l0 == 1);
    CHECK(lpf_set_erosion_element(c, 3) == LPF_OK);
    // the wide call: two erosion iterations are two launches more, with either element
    Ids w = ids_of(2, 40, 4);
    l0 = fake_hip_launches();
    CHECK(run_ids(c, w, 2) == LPF_OK);
    const long long plain = fake_hip_launches() - l0;
    w.erode = 2;
    l0 = fake_hip_launches();
    CHECK(run_ids(c, w, 2) == LPF_OK && fake_hip_launches() - l0 == plain + 2);
    CHECK(lpf_set_erosion_element(c, 5) == LPF_OK);
    l0 = fake_hip_launches();
    CHECK(run_ids(c, w, 2) == LPF_OK && fake_hip_launches() - l0 == plain + 2);
    CHECK(lpf_set_erosion_element(c, 3) == LPF_OK);
    // with a rectangle hint pending (consumed and ignored)
    std::vector<int32_t> rects(2 * 9 * 4, 1);
    CHECK(lpf_set_mask_rects(c, rects.data(), 0, 2, 9) == LPF_OK);
    k.erode = 0;
    CHECK(set_ids(c, k) == LPF_OK && in_force(c, 2));
    // device maps: the call copies sel and nothing else
    long long c0 = fake_hip_copies();
    k = ids_of(2, 9, 4, 1);
    CHECK(set_ids(c, k) == LPF_OK && fake_hip_copies() - c0 == 1);
    k.misalign = true; k.id_bytes = 2;
    c0 = fake_hip_copies();
    CHECK(set_ids(c, k) == LPF_OK && fake_hip_copies() - c0 == 1);
}

static void sizes(lpf_ctx *c)
{
    // growing then shrinking calls on the same context, both ID types, host and device maps
    int n = 0;
    for (int F : {1, 3, 8, 2, 1})
        for (int M : {1, 9, 17, 5, 32}) {
            Ids k = ids_of(F, M, n % 2 ? 4 : 2, n % 3 == 0, M % 3);
            k.misalign = n % 6 == 0;
            ++n;
            CHECK(set_ids(c, k) == LPF_OK && in_force(c, F));
        }
    for (int F : {1, 3, 2, 1})
        for (int M : {1, 33, 256, 40, 5}) {
            Ids k = ids_of(F, M, n % 2 ? 4 : 2, n % 3 == 0, M % 3);
            k.misalign = n % 6 == 0;
            ++n;
            CHECK(run_ids(c, k, F) == LPF_OK);
        }
    CHECK(in_force(c, 1));
    // the 1408 x 376 image: 259 blocks per uint16 frame, 517 per int32 frame
    camera(c, 1408, 376);
    long long l0 = fake_hip_launches();
    CHECK(set_ids(c, ids_of(1, 5, 2)) == LPF_OK && fake_hip_launches() - l0 == 1);
    CHECK(set_ids(c, ids_of(2, 20, 4, 1)) == LPF_OK);
    CHECK(run_ids(c, ids_of(2, 33, 4), 2) == LPF_OK);
    CHECK(run_ids(c, ids_of(1, 256, 2, 1), 1) == LPF_OK);
    {                                                        // more blocks than one launch takes: refused before anything is looked at
        lpf_id_masks in;
        memset(&in, 0, sizeof in);
        in.ids = &in; in.F = INT32_MAX; in.M = 0; in.id_bytes = 2;
        l0 = fake_hip_launches();
        CHECK(lpf_set_masks_ids(c, &in) == LPF_ERR_ARG && err_has("lpf_set_masks_ids: F=2147483647 frames of 529408 pixels are more blocks than one launch takes"));
        CHECK(fake_hip_launches() == l0 && in_force(c, 2));
    }
    camera(c, 37, 23);
}

// a pipelined context with a narrow run owed: lpf_set_masks_ids drains it, lpf_run_wide_ids launches it and runs in order
static void pipelined(lpf_ctx *c)
{
    for (int mode : {2, 4, 0}) {
        CHECK(lpf_set_pipelined(c, mode) == LPF_OK);
        Dev D;
        lpf_outputs o;
        narrow_outputs(D, o, 1, 32, NPTS);
        for (int it = 0; it < 3; ++it) {
            CHECK(set_ids(c, ids_of(1, 5 + 6 * it, it % 2 ? 4 : 2, 0, it)) == LPF_OK);
            CHECK(lpf_run_batch(c, g_pts.data(), g_off, 1, 0, &o) == LPF_OK);        // owed, in modes 2 / 4
            CHECK(run_ids(c, ids_of(1, 40 + it, it % 2 ? 2 : 4, it == 1, it), 1) == LPF_OK);
            CHECK(set_ids(c, ids_of(1, 9, 2, 1)) == LPF_OK);                         // (a device map, with the run above owed nothing)
            CHECK(lpf_run_batch(c, g_pts.data(), g_off, 1, 0, &o) == LPF_OK);
        }
        CHECK(lpf_sync(c) == LPF_OK);
    }
    CHECK(in_force(c, 1));
}

// dense masks through lpf_run_wide after lpf_run_wide_ids on the same context, and ID maps again after them
static void mixed(lpf_ctx *c)
{
    CHECK(run_ids(c, ids_of(2, 40, 2), 2) == LPF_OK);
    {
        Dev D;
        lpf_wide_outputs o;
        wide_outputs(D, o, 2, 70, NPTS);
        std::vector<uint8_t> dense((size_t)2 * 70 * HW, 1);
        lpf_wide_input wi;
        memset(&wi, 0, sizeof wi);
        wi.masks = dense.data(); wi.M = 70; wi.erode_iters = 1;
        const long long l0 = fake_hip_launches();
        CHECK(lpf_run_wide(c, g_pts.data(), g_off, 2, 0, &wi, &o) == LPF_OK && fake_hip_launches() > l0);
    }
    CHECK(run_ids(c, ids_of(2, 256, 4, 1, 1), 2) == LPF_OK);
    CHECK(set_ids(c, ids_of(2, 9)) == LPF_OK);
    {
        std::vector<uint8_t> dense((size_t)2 * 9 * HW, 1);
        CHECK(lpf_set_masks_u8(c, dense.data(), 2, 9, 0, 0) == LPF_OK && in_force(c, 2));
    }
    CHECK(set_ids(c, ids_of(3, 9, 4)) == LPF_OK && in_force(c, 3));
}

int main(int argc, char **argv)
{
    const bool only_ids = argc > 1 && !strcmp(argv[1], "ids"), only_mixed = argc > 1 && !strcmp(argv[1], "mixed");
    lpf_ctx *c = drive_begin();
    if (!only_mixed) {
        state_errors(c);
        refusals(c);
        no_decode(c);
        launches(c);
        sizes(c);
        pipelined(c);
    } else {
        camera(c, 37, 23);
    }
    if (!only_ids) mixed(c);
    lpf_destroy(c);
    return drive_finish("drive_ids", false);
}
