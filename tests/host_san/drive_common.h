// drive_common.h -- what the sanitizer drivers (drive*.cpp) share, and only what at least two of them use: the check macro and the
// error-text predicates, the cameras, exactly-sized output blocks, the run-length masks held the way a careful caller would hold them,
// and the first and last lines of main.  Header-only: every driver is one translation unit, so everything here is static.  Batch
// builders, sections and refusal texts are each driver's own.
#pragma once
#include "../../include/lpf.h"
#include "fake_hip.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int g_fail = 0;
static std::atomic<long long> g_checks{0};                   // CHECKs evaluated (relaxed: drive.cpp's readers run threads)
static lpf_ctx *g_ctx = nullptr;                             // the context whose last error a failed CHECK prints
#define CHECK(cond) do { g_checks.fetch_add(1, std::memory_order_relaxed); \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s  [%s]\n", __FILE__, __LINE__, #cond, lpf_last_error(g_ctx)); ++g_fail; } } while (0)
static inline bool err_is(const char *text) { return strcmp(lpf_last_error(g_ctx), text) == 0; }
static inline bool err_starts(const char *text) { return strncmp(lpf_last_error(g_ctx), text, strlen(text)) == 0; }
static inline bool err_has(const char *text) { return strstr(lpf_last_error(g_ctx), text) != nullptr; }

// ---- cameras
static const double T16[16] = {0, -1, 0, 0.1, 0, 0, -1, 0.2, 1, 0, 0, 0.3, 0, 0, 0, 1};      // KITTI-like: velodyne to rectified camera
static const double K9[9] = {552.5, 0, 682.0, 0, 552.5, 238.7, 0, 0, 1};
static const double IDENT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
static inline void set_camera(lpf_ctx *c, double depth_max = 50.0)                             // the identity camera, 640 x 480
{
    const double K[9] = {500, 0, 320, 0, 500, 240, 0, 0, 1};
    CHECK(lpf_set_camera(c, IDENT, K, 640, 480, 0.0, depth_max) == LPF_OK);
}

// ---- buffers
struct Dev {                      // output ("device") buffers: heap blocks, so that the sanitizer knows their bounds
    std::vector<void *> all;
    template <typename T> T *get(size_t n) { void *p = calloc(n ? n : 1, sizeof(T)); all.push_back(p); return (T *)p; }
    ~Dev() { for (void *p : all) free(p); }
};

// every output of a wide / a narrow run of F frames of npts points with M masks, no boxes, 100 list entries per frame
static inline void wide_outputs(Dev &D, lpf_wide_outputs &o, int F, int M, int npts)
{
    const int64_t n = (int64_t)F * npts;
    const int LW = M > 0 ? (M + 31) / 32 : 1;
    memset(&o, 0, sizeof o);
    o.uv = D.get<int32_t>(2 * n); o.valid_idx = D.get<int64_t>(n); o.uv_valid = D.get<int32_t>(2 * n); o.label_words = D.get<uint32_t>(n * LW);
    o.label_valid_words = D.get<uint32_t>(n * LW); o.inst_idx = D.get<int64_t>((size_t)F * 100); o.inst_cap = 100;
    o.count_mb = D.get<int32_t>((size_t)(M ? M : 1)); o.n_valid = D.get<int64_t>(F); o.n_labelled = D.get<int64_t>(F);
    o.inst_count = D.get<int64_t>((size_t)F * M + 1); o.inst_off = D.get<int64_t>((size_t)F * (M + 1)); o.best_cnt = D.get<int64_t>((size_t)F * M + 1);
    o.best_box = D.get<int32_t>((size_t)F * M + 1); o.inst_overflow = D.get<int32_t>(F);
}
static inline void narrow_outputs(Dev &D, lpf_outputs &o, int F, int M, int npts)
{
    const int64_t n = (int64_t)F * npts;
    memset(&o, 0, sizeof o);
    o.uv = D.get<int32_t>(2 * n); o.label_bits = D.get<uint32_t>(n); o.valid_idx = D.get<int64_t>(n);
    o.inst_idx = D.get<int64_t>((size_t)F * 100); o.inst_cap = 100; o.count_mb = D.get<int32_t>((size_t)(M ? M : 1));
    o.summary = D.get<lpf_frame_summary>(F); o.uv_valid = D.get<int32_t>(2 * n); o.label_valid = D.get<uint32_t>(n);
}

// the state of the context as a caller sees it: F frames of masks of hw pixels in force (lpf_get_label_image fills F * hw words) or none
static inline bool in_force(lpf_ctx *c, int F, int hw)
{
    std::vector<uint32_t> img((size_t)(F > 0 ? F : 1) * hw);
    const int rc = lpf_get_label_image(c, img.data(), 0);
    return F > 0 ? rc == LPF_OK : rc == LPF_ERR_STATE;
}

// `boxes` unit cubes in the dataset's corner order
static inline void unit_cubes(std::vector<double> &corners, size_t boxes)
{
    corners.assign(boxes * 24, 0.0);
    for (size_t b = 0; b < boxes; ++b)
        for (int k = 0; k < 8; ++k) {
            corners[b * 24 + k * 3 + 0] = (k == 1 || k == 2 || k == 5 || k == 6) ? 1.0 : 0.0;
            corners[b * 24 + k * 3 + 1] = (k == 2 || k == 3 || k == 6 || k == 7) ? 1.0 : 0.0;
            corners[b * 24 + k * 3 + 2] = k >= 4 ? 1.0 : 0.0;
        }
}

// ---- run-length masks: one set as a driver builds it ...
struct Rle {
    std::vector<int32_t> runs;          // {start, length} pairs
    std::vector<int64_t> off;
    int F = 1, M = 1, erode = 0, reserved = 0;
};
// ... and as it is handed over: its arrays and its struct in exactly-sized heap blocks, so that a read past either end of one, or
// after release(), is an error here.  release() right after the call: the library has its copies -- scribble, then free.
struct Held {
    int32_t *r = nullptr;
    int64_t *o = nullptr;
    lpf_rle_masks *in = nullptr;
    size_t nr = 0, no = 0;
    explicit Held(const Rle &k) : nr(k.runs.size()), no(k.off.size())
    {
        r = nr ? (int32_t *)malloc(nr * sizeof(int32_t)) : nullptr;
        o = no ? (int64_t *)malloc(no * sizeof(int64_t)) : nullptr;
        if (r) memcpy(r, k.runs.data(), nr * sizeof(int32_t));
        if (o) memcpy(o, k.off.data(), no * sizeof(int64_t));
        in = (lpf_rle_masks *)malloc(sizeof(lpf_rle_masks));
        memset(in, 0, sizeof *in);
        in->runs = r; in->run_off = o; in->F = k.F; in->M = k.M; in->erode_iters = k.erode; in->reserved = k.reserved;
    }
    void release()
    {
        if (r) memset(r, 0xEE, nr * sizeof(int32_t));
        if (o) memset(o, 0xEE, no * sizeof(int64_t));
        memset(in, 0xEE, sizeof *in);
        free(r); free(o); free(in);
        r = nullptr; o = nullptr; in = nullptr;
    }
};
// F * M masks of runs_per_mask runs of `length` pixels each, inside an image of hw pixels
static inline Rle simple(int F, int M, int runs_per_mask, int length, int hw)
{
    Rle k;
    k.F = F; k.M = M;
    k.off.push_back(0);
    for (int i = 0; i < F * M; ++i) {
        for (int j = 0; j < runs_per_mask; ++j) { k.runs.push_back((i * 7 + j * 11) % (hw - length)); k.runs.push_back(length); }
        k.off.push_back((int64_t)k.runs.size() / 2);
    }
    return k;
}

// ---- main's first and last lines
static inline lpf_ctx *drive_begin()
{
    lpf_ctx *c = nullptr;
    CHECK(lpf_create(&c, 0) == LPF_OK && c);
    g_ctx = c;
    return c;
}
// after the driver has destroyed its contexts: the line the tests read, and main's return value
static inline int drive_finish(const char *name, bool with_copies)
{
    g_ctx = nullptr;
    fake_hip_trace_flush();
    fprintf(stderr, "%s: %d failed checks, %lld fake launches, trace hash %016llx", name, g_fail, fake_hip_launches(), fake_hip_trace_hash());
    if (with_copies) fprintf(stderr, ", %lld copies, copy hash %016llx", fake_hip_copies(), fake_hip_copy_hash(0));
    fprintf(stderr, ", %lld checks run\n", g_checks.load());
    return g_fail ? 1 : 0;
}
