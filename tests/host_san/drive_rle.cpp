// drive_rle.cpp -- drives lpf_set_masks_rle's HOST side (lpf_api.hip compiled --offload-host-only against fake_hip.cpp) under
// AddressSanitizer + UndefinedBehaviorSanitizer: every refusal with its message, the state errors, the calls that launch no decode, the
// launches of a call with erosion, 10^5 runs, growing then shrinking calls, and the caller's arrays freed as soon as the call has
// returned (they live in exactly-sized heap blocks, so a read past either end is an error here).  Kernel launches do nothing here
// (fake_hip.cpp): they are counted, and their names go to the FAKE_HIP_TRACE file, by which tests/test_host_sanitized_rle.py checks what
// a call launches; the label images are checked on the GPU by tests/test_gpu_rle.py.
#include "drive_common.h"
#include <climits>

static const int W = 37, H = 23, HW = W * H;

// lpf_set_masks_rle with k as its masks; the arrays and the struct are gone when it returns
static int go(lpf_ctx *c, const Rle &k)
{
    Held h(k);
    const int rc = lpf_set_masks_rle(c, h.in);
    h.release();
    return rc;
}
// drive_common.h's, with this driver's image as the default
static Rle simple(int F, int M, int runs_per_mask, int length = 3, int hw = HW);
static bool in_force(lpf_ctx *c, int F, int hw = HW);

static void state_errors(lpf_ctx *c)
{
    const Rle k = simple(1, 2, 3);
    lpf_rle_masks in;
    memset(&in, 0, sizeof in);
    CHECK(lpf_set_masks_rle(nullptr, &in) == LPF_ERR_ARG);
    CHECK(go(c, k) == LPF_ERR_STATE && err_is("lpf_set_camera must be called before masks (W, H)"));
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    CHECK(go(c, k) == LPF_OK);                                // (buffers exist: a capture could take the launches)
    CHECK(lpf_graph_begin(c) == LPF_OK);
    const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
    CHECK(go(c, k) == LPF_ERR_STATE && err_has("lpf_set_masks_rle cannot be captured into a graph"));
    CHECK(fake_hip_launches() == l0 && fake_hip_copies() == c0);
    lpf_graph *g = nullptr;
    (void)lpf_graph_end(c, &g);                              // (the refusal abandoned the capture, as every error inside one does)
    if (g) lpf_graph_destroy(g);
    CHECK(go(c, k) == LPF_OK && in_force(c, 1));
}

static void refusals(lpf_ctx *c)
{
    CHECK(go(c, simple(2, 3, 2)) == LPF_OK && in_force(c, 2));       // what every refusal below must leave in force
    const long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
    char want[512];
    CHECK(lpf_set_masks_rle(c, nullptr) == LPF_ERR_ARG && err_is("lpf_set_masks_rle: in=NULL"));
    Rle k = simple(1, 2, 1);
    k.F = -1;
    CHECK(go(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_rle: F=-1 M=2 erode_iters=0 reserved=0"));
    k = simple(1, 2, 1); k.M = -1;
    CHECK(go(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_rle: F=1 M=-1 erode_iters=0 reserved=0"));
    k = simple(1, 2, 1); k.erode = -2;
    CHECK(go(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_rle: F=1 M=2 erode_iters=-2 reserved=0"));
    k = simple(1, 2, 1); k.reserved = 7;
    CHECK(go(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_rle: F=1 M=2 erode_iters=0 reserved=7"));
    k = simple(1, 2, 1); k.M = LPF_MAX_MASKS + 1;            // (refused before the arrays are looked at)
    snprintf(want, sizeof want, "set_masks: M=%d masks per frame, a run takes at most LPF_MAX_MASKS = %d (one bit each in label_bits): run the frame "
                                "once per group of %d masks -- everything per point is the same in every pass (pipeline.run_frames does so)",
             LPF_MAX_MASKS + 1, LPF_MAX_MASKS, LPF_MAX_MASKS);
    CHECK(go(c, k) == LPF_ERR_ARG && err_is(want));
    {                                                        // ... the message lpf_set_masks_u8 gives
        uint8_t one = 0;
        CHECK(lpf_set_masks_u8(c, &one, 1, LPF_MAX_MASKS + 1, 0, 0) == LPF_ERR_ARG && err_is(want));
    }
    k = simple(1, 2, 1); k.F = INT32_MAX; k.M = 2;           // (refused before run_off, which would have 2^32 entries, is looked at)
    CHECK(go(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_rle: F * M = 4294967294 masks (at most 2^31 - 1 in one call)"));
    k = simple(1, 2, 1); k.off[0] = 1;
    CHECK(go(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_rle: run_off[0]=1 (must be 0)"));
    k = simple(2, 3, 2); k.off[5] = 7;                       // 0 2 4 6 8 7 12: decreases at k = 4 -> frame 1 mask 1
    CHECK(go(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_rle: run_off decreases at frame 1 mask 1 (7 after 8)"));
    k = simple(1, 2, 1); k.off.clear();
    CHECK(go(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_rle: run_off=NULL with F=1 M=2"));
    k = simple(1, 2, 1); k.runs.clear();
    CHECK(go(c, k) == LPF_ERR_ARG && err_is("lpf_set_masks_rle: runs=NULL with 2 runs"));
    struct Bad { int32_t start, length; } bad[] = {{-1, 3}, {5, -1}, {HW - 2, 3}, {HW, 1}, {INT32_MAX, INT32_MAX}, {0, HW + 1}, {INT32_MIN, 0}};
    for (const Bad &b : bad) {
        k = simple(2, 3, 2);                                 // run 1 of frame 1, mask 2: global run 11
        k.runs[2 * 11] = b.start; k.runs[2 * 11 + 1] = b.length;
        snprintf(want, sizeof want, "lpf_set_masks_rle: frame 1 mask 2 run 1: start=%d length=%d (0 <= start, 0 <= length, start + length <= W*H = %d)",
                 b.start, b.length, HW);
        CHECK(go(c, k) == LPF_ERR_ARG && err_is(want));
    }
    // nothing was queued by any of them, and the masks set before are still in force
    CHECK(fake_hip_launches() == l0 && fake_hip_copies() == c0);
    CHECK(in_force(c, 2));
    // the limits themselves are fine: the whole image, its last pixel, an empty run at the very end
    k = simple(1, 1, 3);
    const int32_t edge[6] = {0, HW, HW - 1, 1, HW, 0};
    memcpy(k.runs.data(), edge, sizeof edge);
    CHECK(go(c, k) == LPF_OK && in_force(c, 1));
}

static void no_decode(lpf_ctx *c)
{
    Rle k;
    // F = 0: as lpf_set_masks_u8 with F = 0 -- no masks in force, nothing queued
    long long l0 = fake_hip_launches(), c0 = fake_hip_copies();
    k = Rle(); k.F = 0; k.M = 5;
    CHECK(go(c, k) == LPF_OK && fake_hip_launches() == l0 && fake_hip_copies() == c0);
    CHECK(in_force(c, 0));
    // M = 0: a zeroed image in force, no decode (run_off has its one entry, or is not given at all)
    l0 = fake_hip_launches(); c0 = fake_hip_copies();
    k = Rle(); k.F = 2; k.M = 0; k.off = {0};
    CHECK(go(c, k) == LPF_OK && fake_hip_launches() == l0 && fake_hip_copies() == c0);
    k.off.clear();
    CHECK(go(c, k) == LPF_OK && fake_hip_launches() == l0);
    CHECK(in_force(c, 2));
    // no run at all, and runs that are all empty: the same, whatever erode_iters asks for
    l0 = fake_hip_launches();
    k = simple(2, 3, 0); k.erode = 2;
    CHECK(go(c, k) == LPF_OK && fake_hip_launches() == l0);
    k = simple(2, 3, 2, 0); k.erode = 1;
    CHECK(go(c, k) == LPF_OK && fake_hip_launches() == l0);
    CHECK(in_force(c, 2));
}

static void launches(lpf_ctx *c)
{
    long long l0 = fake_hip_launches();
    Rle k = simple(2, 9, 4);
    CHECK(go(c, k) == LPF_OK && fake_hip_launches() - l0 == 1);         // the decode
    l0 = fake_hip_launches();
    k.erode = 2;
    CHECK(go(c, k) == LPF_OK && fake_hip_launches() - l0 == 3);         // decode + 2 erosions (none of them fused)
    CHECK(lpf_set_erosion_element(c, 5) == LPF_OK);
    l0 = fake_hip_launches();
    CHECK(go(c, k) == LPF_OK && fake_hip_launches() - l0 == 3);         // ... with the k x k element
    CHECK(lpf_set_erosion_element(c, 1) == LPF_OK);                    // the identity
    l0 = fake_hip_launches();
    CHECK(go(c, k) == LPF_OK && fake_hip_launches() - l0 == 1);
    CHECK(lpf_set_erosion_element(c, 3) == LPF_OK);
    // with a rectangle hint pending (consumed and ignored; the GPU test checks that the next dense masks do not see it)
    std::vector<int32_t> rects(2 * 9 * 4, 1);
    CHECK(lpf_set_mask_rects(c, rects.data(), 0, 2, 9) == LPF_OK);
    k.erode = 0;
    CHECK(go(c, k) == LPF_OK && in_force(c, 2));
}

static void sizes(lpf_ctx *c)
{
    // 10^5 runs, shuffled order, overlaps and repeats; then growing and shrinking calls on the same context
    Rle big;
    big.F = 4; big.M = 32;
    big.off.push_back(0);
    unsigned s = 12345;
    for (int i = 0; i < big.F * big.M; ++i) {
        const int n = i % 3 == 0 ? 0 : 1272 + i % 5;         // ragged, with empty masks
        for (int j = 0; j < n; ++j) {
            s = s * 1664525u + 1013904223u;
            const int start = (int)((s >> 8) % HW), length = (int)((s >> 3) % (HW - start + 1));
            big.runs.push_back(start); big.runs.push_back(length);
        }
        big.off.push_back((int64_t)big.runs.size() / 2);
    }
    CHECK(big.runs.size() / 2 >= 100000);
    CHECK(go(c, big) == LPF_OK && in_force(c, 4));
    for (int F : {1, 3, 8, 2, 1}) {
        for (int M : {1, 9, 17, 5}) {
            Rle k = simple(F, M, F + M, 1 + M);
            k.erode = M % 3;
            CHECK(go(c, k) == LPF_OK && in_force(c, F));
        }
    }
    // one run that is a whole larger image: 530 k pixels in chunks
    CHECK(lpf_set_camera(c, T16, K9, 1408, 376, 0, 50) == LPF_OK);
    Rle full;
    full.F = 1; full.M = 1; full.runs = {0, 1408 * 376}; full.off = {0, 1};
    const long long l0 = fake_hip_launches();
    CHECK(go(c, full) == LPF_OK && fake_hip_launches() - l0 == 1);
    // pipelined modes: what is owed is drained, the masks are in force for the next run
    CHECK(lpf_set_camera(c, T16, K9, W, H, 0, 50) == LPF_OK);
    for (int mode : {2, 4, 0}) {
        CHECK(lpf_set_pipelined(c, mode) == LPF_OK);
        std::vector<float> pts(4 * 1000, 1.0f);
        const int64_t off[2] = {0, 1000};
        std::vector<int32_t> uv(2 * 1000);
        std::vector<uint32_t> bits(1000);
        lpf_outputs o;
        memset(&o, 0, sizeof o);
        o.uv = uv.data(); o.label_bits = bits.data();
        for (int it = 0; it < 3; ++it) {
            Rle k = simple(1, 5 + 6 * it, 3);
            k.erode = it;
            CHECK(go(c, k) == LPF_OK);
            CHECK(lpf_run_batch(c, pts.data(), off, 1, 0, &o) == LPF_OK);
        }
        CHECK(lpf_sync(c) == LPF_OK);
    }
}

int main()
{
    lpf_ctx *c = drive_begin();
    state_errors(c);
    refusals(c);
    no_decode(c);
    launches(c);
    sizes(c);
    lpf_destroy(c);
    return drive_finish("drive_rle", false);
}
