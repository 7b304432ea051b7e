// lpf_api.hip -- host side of liblpf.so: the C ABI of include/lpf.h over the gfx950
// kernels in lpf_kernels.hip.h.  No CPU compute path exists here: every entry point
// either launches HIP kernels or fails with an error code.
#include "lpf_kernels.hip.h"
#include "lpf_wide.hip.h"
#include "lpf_cams.hip.h"
#include "lpf_cams_wide.hip.h"
#include "lpf_frame_wide.hip.h"
#include "lpf_depth_maps.hip.h"
#include "lpf_depth_overlays.hip.h"
#include "lpf_match2d.hip.h"
#include "lpf_assign.hip.h"
#include "lpf_inside.hip.h"
#include "lpf_box_points.hip.h"
#include "lpf_box_views.hip.h"
#include "lpf_first_match.hip.h"
#include "lpf_rle.hip.h"
#include "lpf_ids.hip.h"
#include "../../include/lpf.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <initializer_list>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

// Points per launch up to which a run uses the small geometry: 512-point K1 tiles and 1024-point segments (more,
// shorter blocks and list waves: a single real frame is 107 segments instead of 27).  Measured on single synthetic clouds
// (tools/geometry_probe.py, us per step small / large): 1 M 34.9 / 38.7, 2 M 38.5 / 46.9, 3 M 46.0 / 49.5, 4 M 57.1 / 52.0.
#define LPF_SMALL_LAUNCH (7ll << 19)
// Tail blocks (of four 1024-point segments) up to which the wide form of the tail runs (measured on copies of sample frame 100,
// wide vs narrow: 4 frames = 108 blocks 21.5 vs 26.8 us; 8 frames 24.2 vs 29.2; 12 frames 29.3 vs 33.0; 20 frames = 540 blocks
// 41.0 vs 40.6; 32 frames 55.8 vs 50.6)
#define LPF_WIDE_BELOW 480
#define LPF_FEW_BLOCKS 64           // list blocks of "a frame or two": see lpf_run_batch (count blocks in four parts, 16-row list wave)
// Share of a step launch's K1 tiles (in twentieths) among which the previous run's tail blocks are dealt (see lpf_run_batch)
#ifndef LPF_TAIL_SPREAD_20THS
#define LPF_TAIL_SPREAD_20THS 13
#endif

// K1 tile of a large software-pipelined launch whose tiles read the masks inside their rectangles (LpfDirectRect): 1024 points.
// (2048, what the packed form uses there, needs more registers than the step kernel has -- the exact test of a candidate row computes
//  its pixel again -- and measured slower on real scans even in a form that fitted: 146 frames per step 170 vs 158 us.)
#define LPF_RECT_FUSED_TILE 1024

static_assert(sizeof(lpf_frame_summary) == LPF_SUMMARY_BYTES, "summary layout is shared with lpf_finalize_frame");

namespace {

thread_local std::string g_create_error;

struct DevBuf {                       // grow-only device buffer
    void *p = nullptr;
    size_t cap = 0;
};

// Where the streaming tiles of a run get their label bits (plan_tile_source, once per lpf_run_batch): nowhere (no masks), from the
// packed label image, from the unpacked masks themselves -- all M bytes of a valid point (LpfDirect) -- or from the masks inside their
// rectangles, through the candidate grid (LpfDirectRect).
struct TileSource {
    enum Kind { NONE, PACKED, DIRECT, DIRECT_RECT } kind = NONE;
    bool f32 = false;                 // DIRECT, DIRECT_RECT: the masks' element type (uint8 / float) ...
    int rule = 0;                     // ... and membership rule: 0 (uint8) or 1..3 (float)
    int label_bytes = 4;              // element size of the run's label image (4 without masks)
    const void *img = nullptr;        // what the tiles read (LpfParams::label_img): the label image, or the masks
    const int4 *rects = nullptr;      // the masks' rectangles (LpfParams::rects), DIRECT kinds only: they gate DIRECT tiles too
    bool ride_pack = false;           // mode 4: the pack of the unpacked masks rides in the launch that queues this run
    bool reads_masks() const { return kind == DIRECT || kind == DIRECT_RECT; }
};

}  // namespace

struct lpf_graph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    unsigned long long generation = 0;    // lpf_ctx::generation at capture time
};

#define LPF_NSETS 4                   // scratch sets / box sets in rotation (mode 4 keeps four runs in flight)

struct lpf_ctx {
    bool capturing = false;
    // Bumped by everything a captured graph bakes in and a later call may invalidate: buffer regrowth, table
    // uploads, box / camera / stream / pipelining changes.  lpf_graph_launch refuses a graph of another generation.
    unsigned long long generation = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;

    bool have_camera = false;
    double T[12], K[9], dmin = 0, dmax = 0;
    int W = 0, H = 0;

    // the erosion element (lpf_set_erosion_element): the k x k MORPH_ELLIPSE, its radius and its rows' half-widths as the kernels take
    // them (nibble j = row |dy| = j).  k = 3 is the cross of lpf_pack_erode / lpf_erode_packed / lpf_erode_u8_kernel themselves
    int erode_k = 3, erode_r = 1;
    uint32_t erode_spans = 0x01u;

    // masks -> label images
    DevBuf mask_stage;
    DevBuf ids_stage;                 // lpf_set_masks_ids: [sel | host ids] of the call being decoded (ids_stage_tables)
    DevBuf rle_stage;                 // lpf_set_masks_rle: [runs | work units | run_off] of the call being decoded
    // run-length masks, walked (rle_walk): the checked input and its work units (kept for their capacity).  One record per camera of a
    // multi-camera pass; lpf_set_masks_rle, lpf_run_wide and the two analysis calls use record 0.  Host storage of its own for every
    // camera until the call's host wait.  The tables are staged (rle_stage_tables) in rle_stage by lpf_set_masks_rle, in the pass's own
    // buffers (Wide::rle, Cams::rle) by everyone else
    struct RleIn {
        const lpf_rle_masks *in = nullptr;        // NULL: this camera's masks are dense (or there are none)
        long long Rtot = 0;
        std::vector<int2> units;
    } rle_in[LPF_NSETS];
    // run-length masks of lpf_depth_maps_rle / lpf_first_match_rle (RleCall): the whole batch is checked into rle_in[0]; a range of
    // frames decodes its own slice of it -- the range's runs (the caller's, from `sub.runs` on), run_off rebased to them (off) and the
    // units of those runs with their run index rebased (R.units), as ONE lpf_rle_masks of the range's frames (sub; R.in points at it).
    // One record per range, sized before the first launch and kept until the call returns, past its host wait (the copies of a range's
    // tables read them in stream order); RleCall then clears them and rle_in[0].in, on every way out
    struct RleSlice {
        lpf_rle_masks sub;
        std::vector<int64_t> off;
        RleIn R;
    };
    std::vector<RleSlice> rle_slices;
    // Masks that are set but not packed (no erosion; the next lpf_run* decides, plan_tile_source).  Left by lpf_set_masks_* of a serial
    // context -- host masks in mask_stage, or device masks the caller lends (on_device 2): a launch of sparse frames reads them directly,
    // anything else packs them first -- or of a pipelined one (lent masks only): a fused launch of sparse frames reads them directly, a
    // large one in mode 4 lets their pack ride in its launch (uint8, 16-byte aligned planes: can_ride), anything else packs now
    // (pack_unpacked).  Never both: lpf_set_pipelined packs what it finds.
    struct Unpacked {
        bool valid = false;
        bool pipelined = false;       // left by a pipelined context's lpf_set_masks_*
        const void *masks = nullptr;
        bool f32 = false, can_ride = false;
        int rule = 0, F = 0, M = 0;
        const int4 *rects = nullptr;
        void *label = nullptr;        // the label image they are packed into (label_a of the masks' scratch set)
    };
    // The masks in force: one record, written through the four transitions below only.  The label image and its element size belong
    // to scratch set `set`: a call that sets masks names its set first (begin), and every later writer works on that set's buffers.
    struct Masks {
        int F = 0, M = 0;             // 0 frames = no masks set
        int set = 0;                  // the scratch set whose label_a / label_b hold the label image
        void *img = nullptr;          // the label image: that set's label_a or (after an erosion) label_b
        int bytes = 4;                // its element size: 1 (M <= 8), 2 (M <= 16) or 4
        Unpacked unpacked;
        void forget_unpacked() { unpacked = Unpacked(); }
        void drop() { F = 0; M = 0; forget_unpacked(); }                // none in force (img stays: nothing reads it while F is 0)
        // a call that sets masks begins: none in force, what it sets goes to set s.  Lent masks that a pipelined lpf_set_masks_* left
        // unpacked stay on record (the callers say why)
        void begin(int s) { F = 0; M = 0; img = nullptr; set = s; if (!unpacked.pipelined) forget_unpacked(); }
        void packed(int F_, int M_, void *image, int b) { F = F_; M = M_; img = image; bytes = b; }     // in force, packed into `image`
        // the masks the caller has just recorded in `unpacked` are in force: the next run decides; a pack writes elements of b bytes
        // (image: on record meanwhile, or NULL)
        void left_unpacked(void *image, int b) { F = unpacked.F; M = unpacked.M; img = image; bytes = b; }
    } masks;

    // One set of box tables, and the job (LpfBoxJob) that fills them.  F, job_valid, used and last_ref are written by the methods
    // below and by lpf_ctx::Boxes only.
    struct BoxSet {
        int F = 0, oriented = 1;                  // 0 frames = no boxes here
        std::vector<int32_t> box_off;             // F+1
        std::vector<LpfBoxFrame> h_bframes, h_bframes_dev;   // per-frame records: being built / in HBM (F > 1 only)
        std::vector<long long> cand_off;          // [F] first word of frame f's grid
        size_t cand_words = 0;                    // words of the whole grid
        int max_words = 1;                        // 64-bit words per cell of the frame with the most boxes
        DevBuf boxp;                              // [Btot][16] double
        DevBuf boxq;                              // [Btot][8] float conservative AABB
        DevBuf cand;                              // ground grids: LPF_GRID_WORDS words per 64 boxes of a frame
        DevBuf corners;                           // [Btot][8][3] velodyne-frame corners the tables were built from (lpf_set_boxes_cam0's host output corners_velo)
        DevBuf enabled;                           // [Btot] bytes: 0 = dropped by filter_visible_bboxes (lpf_set_boxes_cam0; its host output visible)
        DevBuf aux;                               // lpf_set_boxes_cam0 for host callers: projected 2D boxes + front counts
        DevBuf bframes;                           // [F] LpfBoxFrame
        DevBuf stage;                             // corners copied from the caller (host memory, or device memory that is not lent)
        bool used = false;                        // a run has been queued with these tables since they were set
        long long last_ref = -1;                  // ... the last such run (Boxes::run_seq)
        bool job_valid = false;                   // tables not built yet: the job rides in the next run's launch (or is launched by it)
        LpfBoxJob job;
        void clear() { F = 0; box_off.clear(); job_valid = false; }      // no boxes here (the buffers stay: nothing reads them while F is 0)
        void begin() { clear(); used = false; last_ref = -1; }           // a call that sets boxes starts on this set: no run has read what it will hold
        void shaped(const int32_t *off, int F_, int oriented_) { box_off.assign(off, off + F_ + 1); F = F_; oriented = oriented_ ? 1 : 0; }
        int total() const { return F ? box_off[(size_t)F] : 0; }         // boxes of all frames
        // The fields every job has: corners from src (velodyne frame unless the caller adds cam0), this set's tables and its copy of the
        // corners as outputs.  The job waits for the launch that takes it.
        LpfBoxJob &new_job(const double *src)
        {
            memset(&job, 0, sizeof job);
            job.src = src; job.oriented = oriented; job.F = F; job.chunks = max_words;
            job.bframes = (const LpfBoxFrame *)bframes.p;
            if (F > 0) job.frame0 = h_bframes[0];
            job.boxp = (double *)boxp.p; job.boxq = (float *)boxq.p; job.cand = (unsigned long long *)cand.p;
            job.corners_keep = (double *)corners.p;
            job_valid = true;
            return job;
        }
        bool job_ready() const { return job_valid && total() > 0; }     // a job worth launching
        bool take_job() { const bool ready = job_ready(); job_valid = false; return ready; }      // by the launch that carries it, if it is ready
    };
    // Boxes.  A ring of box sets: in the software-pipelined modes the tail that counts into the boxes of run i executes one
    // or two launches after run i was queued, so a lpf_set_boxes* for the NEXT run must not touch the tables run i's tail is
    // going to read -- it takes the next set of the ring instead (no drain, no synchronisation), and the preparation of its
    // tables (LpfBoxJob) rides in that run's launch.  Serial mode stays on one set: the stream orders everything.
    struct Boxes {
        BoxSet ring[LPF_NSETS];
        int cur = 0;                  // the set in force
        long long run_seq = 0;        // runs queued so far
        BoxSet &in_force() { return ring[cur]; }                         // the set a run or an analysis call reads
        // The set a lpf_set_boxes* call writes.  Pipelined (fused; depth: launches from the one that queues a run to the one with its
        // tail): the next one of the ring once a run has used the current one -- that run's tail has yet to read its tables -- and
        // *owed says that the last reader of the set's old tables may not have been LAUNCHED yet: the caller launches what the
        // pipeline owes before it rewrites them (stream order does the rest; with one set per run and four sets it never happens).
        // In order: the current set.  (Never inside a graph capture: see Pipeline::set_now.)
        BoxSet &set_for_write(bool fused, int depth, bool *owed)
        {
            *owed = false;
            if (fused) {
                if (ring[cur].used) {
                    ring[cur].job_valid = false;           // (cannot be: a run launches the job of the set it uses)
                    cur = (cur + 1) % LPF_NSETS;
                }
                *owed = ring[cur].last_ref >= 0 && ring[cur].last_ref + depth >= run_seq;
            }
            return ring[cur];
        }
        void claimed_by_run() { ring[cur].used = true; ring[cur].last_ref = run_seq++; }     // a run has been queued that reads the set in force
        void drop() { for (BoxSet &B : ring) B.clear(); }                // none in force, in any set
    } boxes;

    // Scratch of one in-flight run, including its geometry tables (frame records, per-segment frame records, tail block table):
    // a run whose batch shape differs from the previous one's uploads its own tables -- through the pinned ring below, in stream
    // order, without waiting -- instead of draining the pipeline to rewrite shared ones.  A launch of ONE frame needs no table.
    struct Scratch {
        DevBuf vbal, mbal, seg_tab, grp_tab, frm_tab, seg_pre, cnt, mlist;
        DevBuf label_a, label_b;      // label images [F][H][W] uint32 (b = erosion ping-pong); which one is current: lpf_ctx::Masks
        DevBuf rgrid;                 // candidate grid of the masks' rectangles (LpfDirectRect tiles), [F][cells] uint32
        DevBuf rects;                 // lpf_set_mask_rects from host memory: the copy this set's run reads (its tiles may run a launch later)
        DevBuf out_stage;             // what a pipelined run needs though its caller left it out (narrow_bind): written by this run's tiles,
                                      // read by its tail a launch later, while the next run's tiles write theirs -- so one per set
        DevBuf tab;                   // [frames | segs | blks]
        std::vector<LpfFrame> tab_frames;         // the frame records `tab` was built from (empty: none) ...
        int tab_csplit = 0;                       // ... and its count blocks per (group, word): the key of the tables (narrow_tables)
        size_t o_segs = 0, o_blks = 0, o_cblks = 0;
    } sc[LPF_NSETS];
    struct Pending {                  // a run, as the step launches that carry its roles take it
        bool valid = false;
        LpfParams P;
        bool pre = false;                 // its prefixes come from the scan kernel
        int ntail = 0;                    // tail blocks
        int nk1 = 0;                      // K1 tiles
        TileSource src;                   // where its tiles get their label bits
    };
    // Software-pipelined modes (lpf_set_pipelined 2 / 4): the mode, the scratch set of the next fused run and what earlier runs still
    // owe.  The tail of the last run and the summaries of the one before ride in the next run's launch (lpf_step_t) -- in mode 4 the
    // last run's streaming kernel too (k1) -- or are launched by flush_pending(); queue_step alone moves a run from role to role.
    struct Pipeline {
        bool fused = false;           // pipelined: one launch per run (modes 2 / 4)
        // Mode 4: the mask pack rides as well -- the launch of run i carries the pack of run i's masks, the K1 tiles of run i-1
        // (k1), the tail of run i-2 and the summaries of run i-3; four scratch sets.
        bool defer = false;
        int parity = 0;               // the scratch set of the next fused run
        Pending k1, tail, fin;
        bool owes() const { return k1.valid || tail.valid || fin.valid; }
        int sets() const { return defer ? 4 : 3; }        // scratch sets in rotation
        int depth() const { return defer ? 2 : 1; }       // launches from the one that queues a run to the one with its tail
        // The scratch set that masks and rectangles set NOW go to: the next fused run's, in order set 0.  (A graph capture has no say:
        // lpf_graph_begin refuses a pipelined context, and lpf_set_pipelined goes through sync_all, which refuses inside a capture.)
        int set_now() const { return fused ? parity : 0; }
        int run_set(bool run_fused) const { return run_fused ? parity : 0; }      // a run's set: fused or not is that run's own decision
        // a fused run whose mask pack rides (src) may not share its launch with the tiles that wait in k1 (why: lpf_run_batch)
        bool must_drain_before(const TileSource &src) const { return defer && k1.valid && src.ride_pack && (k1.src.reads_masks() || k1.src.label_bytes != src.label_bytes); }
        bool next_carries_tiles() const { return !defer || (k1.valid && k1.nk1 > 0); }    // the launch that queues the next fused run has tiles
    } pipe;
    // lpf_get_stats: [0] host waits, [1] drains (owed work launched outside a run), [2] uploads through the pinned ring, [3] step
    // launches, [4] box jobs launched as a kernel of their own, [5] box jobs that rode in a step launch, [6] blocking uploads,
    // [7] lpf_run_frame_wide jobs whose masks were read directly (lpf_wide_direct_project)
    long long stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // lpf_set_mask_rects: rectangles for the NEXT lpf_set_masks_* (device pointer: the caller's, or rects_buf), consumed by it
    DevBuf resize_buf;                // lpf_resize_masks_u8: weight tables (+ staging for host callers)
    const int4 *rects_pending = nullptr; int rects_F = 0, rects_M = 0;
    DevBuf lab_clk;                   // LPF_LAB builds (lpf_lab_role_clock): 6 roles x 5 counters, or empty
    long long lab_budget = 0;         // LPF_LAB builds (lpf_lab_set_range_limits): a range's staging budget and most items, 0 = the product's
    int lab_max_items = 0, lab_ranges = 0;   // ... and the ranges the last batched call planned (lpf_lab_last_ranges)
    int geometry = 0;                 // LPF_LAB builds (lpf_set_geometry): 0 by launch size, 1 small, 2 large, 3 large + scan-kernel prefixes, 4 small + narrow tail

    // Pinned host ring for small uploads (tables, host corners) that must not block: the source of an asynchronous copy has to
    // stay put until the copy has executed, so each upload takes the next piece of the ring; a quarter of the ring is reused only
    // after an event recorded when it was left has completed (one event per 2 MB of uploads, not per upload).
    struct PinRing { char *base = nullptr; size_t cap = 0, head = 0; hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; bool rec[4] = {false, false, false, false}; } ring;

    struct PinBack { char *p = nullptr; size_t cap = 0; } pin_back;   // page-locked landing area of small results (lpf_prepare_boxes)

    // host-io staging
    DevBuf pib_box, pib_pts, pib_out, boxprep, dimg, coll;
    DevBuf st_pts;                    // staged points of a host caller (lpf_run_batch, lpf_depth_image)
    DevBuf out_stage;                 // lpf_run_batch: staged outputs of a host caller, and what an IN-ORDER run needs though its caller left it out
                                      // (narrow_bind); a pipelined run keeps those in its scratch set (Scratch::out_stage)
    std::vector<LpfFrame> h_frames;   // frame records being built (narrow_layout)
    std::vector<char> h_tab;          // [frames | segs | blks] being built

    // lpf_run_wide: its own buffers (the narrow masks, label images and staging stay as they are)
    struct Wide { DevBuf tab, masks, rects, rle, ids, planes_a, planes_b, flags, ccnt, cpre, fcnt, midx, mwords, mpts, cnt, pts, out; } wide;
    // lpf_run_cams: camera c's box tables, label images, staged masks / rectangles and host-output staging (grow-only, allocated on
    // first use); its counters and geometry tables are scratch set c's
    struct Cams { BoxSet bx[LPF_NSETS]; DevBuf label_a[LPF_NSETS], label_b[LPF_NSETS], masks[LPF_NSETS], rects[LPF_NSETS], rle[LPF_NSETS], out[LPF_NSETS], pts; } cams;
    // lpf_run_cams_wide: camera c's lpf_run_wide buffers (cam[c]: staged masks, planes, scratch, host-output staging), the pass's frame
    // tables and staged points (grow-only, allocated on first use); its box tables are lpf_run_cams' (cams.bx[c])
    struct CamsWide { Wide cam[LPF_NSETS]; DevBuf tab, pts; } camsw;
    // lpf_depth_maps: frame offsets, a chunk's winner planes, counters, staged masks and rectangles, staged points, host-output staging
    // and (with erosion, or run-length masks) lpf_run_wide's label planes in pack.planes_* and a range's run tables in pack.rle
    // (grow-only, allocated on first use)
    struct DepthMaps { Wide pack; DevBuf foff, win, cnt, in, pts, out; } dmaps;
    // the analysis calls, each its own: the frame table, staged host points, staged host inputs (lists, detections, corners, segmented
    // images), staged host outputs (grow-only, allocated on first use; a call leaves empty what it does not stage)
    struct CallBufs { DevBuf tab, pts, in, out; } dovl, m2d, insd, bpts, bviews;       // lpf_depth_overlays, lpf_match_2d, lpf_inside_masks, lpf_box_points, lpf_box_views
    CallBufs asgn;                    // lpf_assign_costs / lpf_assign_2d (pts: the scratch matrices, live-column maps and counts of a range)
    // lpf_first_match: the analysis calls' four (tab: the frame offsets; in: a range's staged masks and colours) and its scratch -- a
    // range's 4-byte codes when the dense output is not asked for, and its tile counters
    // (lpf_first_match_rle: a range's label planes [fc][LW][mh][mw] in pack.planes_a, its run tables in pack.rle)
    struct FirstMatch : CallBufs { DevBuf code, tiles; Wide pack; } fmat;

    // optional event bracketing of K1 (lpf_profile_*)
    bool profiling = false;
    std::vector<hipEvent_t> ev;       // pairs: ev[2i] before, ev[2i+1] after
    size_t ev_used = 0;               // pairs recorded since the last reset
};

namespace {

int fail(lpf_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    if (c && c->capturing) {              // an error inside a capture ends it: the stream must not stay in capture mode
        c->capturing = false;
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(c->stream, &g);
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        c->err += " [the graph capture in progress was abandoned]";
    }
    return code;
}

#define LPF_HIP(c, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail((c), LPF_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                     \
    } while (0)

// ---- one dispatcher per template axis of the kernels ----------------------------------------------------------------------------------
// Each hands a tag to a generic lambda, which launches (or calls on) the instantiation the tag names; only what a helper names here is
// instantiated, so the library carries no kernel that no call can select.
template <typename T, int RULE> struct MaskKind { typedef T elem; static constexpr int rule = RULE; };
template <typename T> struct TypeTag { typedef T type; };
template <int N> using Rows = std::integral_constant<int, N>;
template <bool B> using Flag = std::integral_constant<bool, B>;

// the masks' element type and membership rule: uint8 under rule 0 (lpf_set_masks_u8), float under rules 1..3 (lpf_set_masks_f32's
// binarize + 1) -- the four pairs the interface can ask for
template <typename Fn> auto with_rule(bool f32, int rule, Fn &&fn)
{
    if (!f32) return fn(MaskKind<uint8_t, 0>());
    if (rule == 1) return fn(MaskKind<float, 1>());
    if (rule == 2) return fn(MaskKind<float, 2>());
    return fn(MaskKind<float, 3>());
}

// the element type of a label image of `bytes` per pixel: 1 (M <= 8), 2 (M <= 16) or 4
template <typename Fn> auto with_label(int bytes, Fn &&fn)
{
    if (bytes == 1) return fn(TypeTag<uint8_t>());
    if (bytes == 2) return fn(TypeTag<uint16_t>());
    return fn(TypeTag<uint32_t>());
}

template <typename Fn> auto with_flag(bool on, Fn &&fn)
{
    if (on) return fn(Flag<true>());
    return fn(Flag<false>());
}

// The forms of a run's streaming tiles: fn(tile type, rows of 256 points, scan-kernel tail).  STEP: lpf_step_t's (tiles of 512 / 1024 /
// 2048 points, the riding tail with or without the scan kernel's prefixes); else lpf_k1_project_t's (512 / 1024, no tail).  Packed
// tiles come in every size; tiles that read all M mask bytes of a point (LpfDirect) in 512 points only; tiles that read the masks
// inside their rectangles (LpfDirectRect) for uint8 rule 0 and float rule 1, in 1024 points -- they need a launch beyond the small
// geometry, whose tiles are 1024 points in order and LPF_RECT_FUSED_TILE fused -- and never beside a scan-kernel tail (launch_step).
static_assert(LPF_RECT_FUSED_TILE == 1024, "LpfDirectRect tiles are instantiated for 1024 points only");
template <bool STEP, typename Fn> void with_tile_form(const TileSource &src, int rows, bool scan_tail, Fn &&fn)
{
    auto tail = [&](auto lt, auto rw) {
        if (STEP && scan_tail) fn(lt, rw, Flag<STEP>()); else fn(lt, rw, Flag<false>());
    };
    if (src.kind == TileSource::DIRECT_RECT) {
        if (!src.f32) fn(TypeTag<LpfDirectRect<uint8_t, 0>>(), Rows<4>(), Flag<false>());
        else fn(TypeTag<LpfDirectRect<float, 1>>(), Rows<4>(), Flag<false>());
    } else if (src.kind == TileSource::DIRECT) {
        with_rule(src.f32, src.rule, [&](auto kind) { tail(TypeTag<LpfDirect<typename decltype(kind)::elem, decltype(kind)::rule>>(), Rows<2>()); });
    } else {                                               // (packed tiles; without masks, those for 4-byte labels)
        with_label(src.label_bytes, [&](auto lt) {
            if (rows == 2) tail(lt, Rows<2>());
            else if (STEP && rows == 8) tail(lt, Rows<STEP ? 8 : 4>());
            else tail(lt, Rows<4>());
        });
    }
}

hipError_t host_wait(lpf_ctx *c)        // the host blocks until the context's stream is idle (counted: lpf_get_stats)
{
    ++c->stats[0];
    return hipStreamSynchronize(c->stream);
}

// the narrow tail kernel (serial mode)
void launch_tail(hipStream_t st, const LpfParams &P, int ntail, bool pre)
{
    if (pre) hipLaunchKernelGGL((lpf_tail_t<true>), dim3((unsigned)ntail), dim3(LPF_BLOCK), 0, st, P);
    else hipLaunchKernelGGL((lpf_tail_t<false>), dim3((unsigned)ntail), dim3(LPF_BLOCK), 0, st, P);
}

// camera-dependent fields of a box job: filled when the job is launched, so a job that waits for its run always sees the
// camera of that run
void box_job_camera(LpfBoxJob &J, const double K[9], int W, int H)
{
    memcpy(J.K, K, sizeof J.K);
    J.W = W; J.H = H;
}

// blocks of a set's box job: frames x 64-box chunks of the frame with the most boxes
int box_job_blocks(const lpf_ctx::BoxSet &B) { return B.F * B.job.chunks; }

// the box job of a set as a kernel of its own, on the context's stream (serial mode, graph capture, drains, a camera of lpf_run_cams),
// in the camera K, W, H: the context's, unless the caller names another
int launch_box_job(lpf_ctx *c, lpf_ctx::BoxSet &B, const double K[9], int W, int H)
{
    if (!B.take_job()) return LPF_OK;
    box_job_camera(B.job, K, W, H);
    ++c->stats[4];
    hipLaunchKernelGGL(lpf_box_job_kernel, dim3((unsigned)box_job_blocks(B)), dim3(LPF_BLOCK), 0, c->stream, B.job);
    LPF_HIP(c, hipGetLastError());
    return LPF_OK;
}
int launch_box_job(lpf_ctx *c, lpf_ctx::BoxSet &B) { return launch_box_job(c, B, c->K, c->W, c->H); }

// One launch of lpf_step_t: the streaming tiles of run K, the tail blocks of run Q dealt out among them, the summaries of
// run R, the box job X of the run being queued (a block per frame, in front) and -- mode 4 -- the pack of that run's masks, waiting
// in c->masks.unpacked, behind the tiles (cur: the source of the run being queued, NULL in a drain; its pack rides if it says so, with label
// elements of its size -- K's when K is there: the host keeps the two equal).  Any of the roles may be absent.  `after` is recorded
// behind the launch.
int launch_step(lpf_ctx *c, const lpf_ctx::Pending &KK, const lpf_ctx::Pending &Q, const lpf_ctx::Pending &R, const TileSource *cur,
                lpf_ctx::BoxSet *XB, hipEvent_t after, const LpfRectJob *RG = nullptr)
{
    static const LpfParams none = {};                      // unused roles get a well-formed struct
    static const LpfBoxJob nojob = {};
    if (KK.valid && KK.src.kind == TileSource::DIRECT_RECT && Q.valid && Q.pre) {
        // tiles that read the masks inside their rectangles exist without the scan-kernel form of the riding tail (frames of more than
        // 16.7 M points: rare): that tail and the summaries go in a launch of their own, ahead of the tiles
        static const lpf_ctx::Pending nobody = lpf_ctx::Pending();
        TileSource no_pack = cur ? *cur : TileSource();
        no_pack.ride_pack = false;
        int rc_ = launch_step(c, nobody, Q, R, cur ? &no_pack : nullptr, nullptr, nullptr);
        if (rc_) return rc_;
        return launch_step(c, KK, nobody, nobody, cur, XB, after, RG);
    }
    const bool ride = cur && cur->ride_pack;
    const LpfParams &KP = KK.valid ? KK.P : none, &QP = Q.valid ? Q.P : none, &RP = R.valid ? R.P : none;
    // (a launch without tiles is instantiated as packed tiles with the label elements of the run being queued)
    TileSource tiles = KK.src;
    if (!KK.valid) { tiles = TileSource(); tiles.label_bytes = cur ? cur->label_bytes : 4; }
    LpfStepLayout Y;
    LpfPackJob J;
    memset(&J, 0, sizeof J);
    Y.nfin = R.valid ? R.P.F : 0;
#ifdef LPF_LAB
    Y.clk = (unsigned long long *)c->lab_clk.p;
#endif
    Y.nfin8 = (Y.nfin + 7) & ~7;
    const bool boxes = XB && XB->take_job();
    if (boxes) box_job_camera(XB->job, c->K, c->W, c->H);
    const LpfBoxJob &XJ = boxes ? XB->job : nojob;
    Y.nbox = boxes ? box_job_blocks(*XB) : 0;
    Y.nbox8 = (Y.nbox + 7) & ~7;
    static const LpfRectJob norect = {};
    const LpfRectJob &GJ = RG ? *RG : norect;
    Y.nrg = RG ? RG->F * RG->bpf : 0;
    Y.nrg8 = (Y.nrg + 7) & ~7;
    Y.ntail = Q.valid ? Q.ntail : 0;
    Y.nk1 = KK.valid ? KK.nk1 : 0;
    Y.npack = 0;
    if (ride) {
        const lpf_ctx::Unpacked &U = c->masks.unpacked;
        J.masks = (const uint8_t *)U.masks; J.label = U.label; J.M = U.M; J.hw = (long long)c->H * c->W;
        J.rects = U.rects; J.W = c->W;
        J.total16 = (long long)U.F * (J.hw / 16);
        Y.npack = (int)((J.total16 + LPF_BLOCK - 1) / LPF_BLOCK);
    }
    const int nk1_pad = (Y.nk1 + 7) & ~7;
    Y.nper = (Y.ntail + 7) / 8;
    Y.kper = Y.nk1 > 0 ? 8 : 0;                            // (a drain launch without tiles: the tail blocks alone, no empty tile slots)
    if (Y.nper > 0 && Y.nk1 > 0) {                                      // spread the tail blocks over the first two thirds of the tiles (same box,
        // us per step at 40 / 50 / 60 / 70 / 80 / 90 %: 105.6 / 103-105.6 / 99.5-101.6 / 100.3-101.1 / 101.8-102.3 / 102.3-102.5;
        // again with the pack riding, 40 / 50 / 65 / 80 / 95 %: 95.4 / 95.6-95.9 / 91.4-92.0 / 93.2-93.3 / 93.9:
        // early enough that the last tail blocks do not outlive the tiles, late enough not to crowd the start)
        const long long k = ((long long)nk1_pad * LPF_TAIL_SPREAD_20THS / 20 / 8) / Y.nper;
        Y.kper = (int)(k < 1 ? 1 : k) * 8;
    }
    const long long rest = (long long)nk1_pad - (long long)Y.nper * Y.kper;
    Y.rest = (int)(rest > 0 ? rest : 0);
    const long long grid = (long long)Y.nfin8 + Y.nbox8 + Y.nrg8 + (long long)Y.nper * (Y.kper + 8) + Y.rest + Y.npack;
    if (grid > 0) {
        const dim3 gs((unsigned)grid);
        ++c->stats[3];
        if (boxes) ++c->stats[5];
        with_tile_form<true>(tiles, KP.tile_pts >> 8, Q.valid && Q.pre, [&](auto lt, auto rw, auto pr) {
            with_flag(boxes, [&](auto bx) {
                hipLaunchKernelGGL((lpf_step_t<decltype(rw)::value, LPF_K1_FLAGS, typename decltype(lt)::type, decltype(pr)::value, decltype(bx)::value>),
                                   gs, dim3(LPF_BLOCK), 0, c->stream, KP, QP, RP, Y, J, XJ, GJ);
            });
        });
        LPF_HIP(c, hipGetLastError());
    }
    if (after) LPF_HIP(c, hipEventRecord(after, c->stream));
    if (KK.valid && KK.pre && KK.P.nseg_total > 0) {       // frames beyond 64 groups: their prefixes are scanned before the tail rides
        hipLaunchKernelGGL(lpf_scan_segments, dim3(KK.P.F), dim3(LPF_BLOCK), 0, c->stream, KK.P);
        LPF_HIP(c, hipGetLastError());
    }
    return LPF_OK;
}

// a run as launch_step takes it (the fields: lpf_ctx::Pending)
lpf_ctx::Pending pending_run(const LpfParams &P, bool pre, int ntail, int nk1, const TileSource &src)
{
    return lpf_ctx::Pending{true, P, pre, ntail, nk1, src};
}

// The pipeline's one rotation: a step launch with the tiles of run K, the tail of run Q and the summaries of run R, after which each
// of them has moved on by one role.  cur: the run being queued -- its tiles go into this launch (mode 2) or wait for the next (mode 4),
// its mask pack rides if cur->src says so -- or NULL in a drain: the same launches, with fewer roles each time.
int queue_step(lpf_ctx *c, const lpf_ctx::Pending *cur, lpf_ctx::BoxSet *XB, hipEvent_t after, const LpfRectJob *RG)
{
    lpf_ctx::Pipeline &PL = c->pipe;
    const bool wait = cur && PL.defer;
    const lpf_ctx::Pending K = (cur && !wait) ? *cur : PL.k1, Q = PL.tail, R = PL.fin;
    int rc_ = launch_step(c, K, Q, R, cur ? &cur->src : nullptr, XB, after, RG);
    if (rc_) return rc_;
    PL.fin = Q;                            // its tail has just been launched: summaries in the next launch
    PL.tail = K;
    if (wait) PL.k1 = *cur; else PL.k1.valid = false;
    return LPF_OK;
}

// software-pipelined modes: launch what earlier runs still owe; a box job that was waiting for its run goes with the first of those
// launches (or alone)
int flush_pending(lpf_ctx *c)
{
    lpf_ctx::BoxSet *XB = &c->boxes.in_force();
    int rc_;
    if (c->pipe.owes()) ++c->stats[1];
    while (c->pipe.owes())
        if ((rc_ = queue_step(c, nullptr, XB, nullptr, nullptr))) return rc_;
    return launch_box_job(c, *XB);
}

int sync_all(lpf_ctx *c)                // the stream idle, nothing owed: any table / buffer may be rewritten or freed
{
    if (c->capturing)
        return fail(c, LPF_ERR_STATE, "this call needs a synchronisation or (re)allocation, which cannot be captured into a graph: "
                                      "run the same shapes once before lpf_graph_begin");
    { int rc_ = flush_pending(c); if (rc_) return rc_; }
    LPF_HIP(c, host_wait(c));
    for (bool &r : c->ring.rec) r = false;                  // every upload has executed
    return LPF_OK;
}

// grow-only; new memory is zeroed (the self-cleaning counters rely on it)
int reserve(lpf_ctx *c, DevBuf &b, size_t bytes, bool zero = false)
{
    if (bytes <= b.cap && b.p) return LPF_OK;
    if (c->capturing) return fail(c, LPF_ERR_STATE, "allocation inside graph capture: run the same shapes once before lpf_graph_begin");
    if (bytes == 0) bytes = 256;
    if (b.p) {
        int rc_ = sync_all(c);
        if (rc_) return rc_;
        LPF_HIP(c, hipFree(b.p));
        b.p = nullptr; b.cap = 0;
        ++c->generation;                  // a captured graph may hold the freed pointer
    }
    const size_t want = bytes + bytes / 4;        // headroom against regrowth
    if (hipMalloc(&b.p, want) != hipSuccess) {
        b.p = nullptr;
        return fail(c, LPF_ERR_NOMEM, "hipMalloc(%zu) failed", want);
    }
    b.cap = want;
    if (zero) LPF_HIP(c, hipMemsetAsync(b.p, 0, want, c->stream));
    return LPF_OK;
}

void release(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Where the arrays of a call live: the caller's device memory, or ONE staging buffer.  add(): one line per array -- the field of the
// kernel-parameter struct (or a local pointer) that is to point at it, the caller's pointer (NULL: not given / not asked for), the bytes
// of an element, the elements of the largest range the call will stage at once (of the whole batch, for a call that does not cut it),
// and whether the call needs the array itself when the caller left it out.  `host` says where the arrays declared next are: a call
// whose arrays come from both sides sets it between add()s.  commit(): a device caller's array is lent -- the field gets the caller's
// pointer; a host caller's, and one the call needs though the caller left it out, is a 256-byte aligned piece of the buffer, reserved
// here; anything else is NULL.  in() / back(): the copies of the staged arrays from / to the host caller, queued on the stream -- all of
// every array, or per array the elements [first, first + count) of the caller's, which lie at the start of the staged piece.  Fixed
// capacity, nothing on the heap: it sits on the per-step path of a pipelined stream.
struct Span { size_t first, count; };
struct Stage {
    enum { CAP = 20 };
    struct Item { void *field; void *user; size_t esz, most, off; bool staged; } item[CAP];
    int n = 0;
    bool host;
    char *base = nullptr;
    explicit Stage(bool host_ = false) : host(host_) {}
    template <typename T> void add(T *&field, const void *user, size_t esz, size_t most, bool needed = false)
    {
        if (n < CAP) item[n] = Item{&field, const_cast<void *>(user), esz, most, 0, user ? host : needed};
        ++n;
    }
    int commit(lpf_ctx *c, DevBuf &buf)
    {
        if (n > CAP) return fail(c, LPF_ERR_STATE, "Stage: %d arrays, room for %d", n, (int)CAP);
        size_t total = 0;
        bool any = false;
        for (int i = 0; i < n; ++i) {
            Item &t = item[i];
            if (!t.staged) continue;
            any = true;
            t.off = total;
            total += align256(t.esz * t.most);
        }
        int rc;
        if (any && (rc = reserve(c, buf, total))) return rc;
        base = (char *)buf.p;
        for (int i = 0; i < n; ++i) {
            void *p = item[i].staged ? (void *)(base + item[i].off) : item[i].user;
            memcpy(item[i].field, &p, sizeof p);           // (the field is a pointer of some type: written as the bytes of one)
        }
        return LPF_OK;
    }
    int in(lpf_ctx *c, std::initializer_list<Span> spans = {}) const { return copies(c, spans, true); }
    int back(lpf_ctx *c, std::initializer_list<Span> spans = {}) const { return copies(c, spans, false); }

private:
    int copies(lpf_ctx *c, std::initializer_list<Span> spans, bool up) const
    {
        if (spans.size() && (int)spans.size() != n) return fail(c, LPF_ERR_STATE, "Stage: %d spans for %d arrays", (int)spans.size(), n);
        for (int i = 0; i < n; ++i) {
            const Item &t = item[i];
            const Span r = spans.size() ? spans.begin()[i] : Span{0, t.most};
            const size_t bytes = r.count * t.esz;
            if (!t.staged || !t.user || !bytes) continue;
            if (r.count > t.most) return fail(c, LPF_ERR_STATE, "Stage: array %d: %zu elements, staged for %zu", i, r.count, t.most);
            char *u = (char *)t.user + r.first * t.esz, *d = base + t.off;
            if (up) LPF_HIP(c, hipMemcpyAsync(d, u, bytes, hipMemcpyHostToDevice, c->stream));
            else LPF_HIP(c, hipMemcpyAsync(u, d, bytes, hipMemcpyDeviceToHost, c->stream));
        }
        return LPF_OK;
    }
};

int use_device(lpf_ctx *c)
{
    LPF_HIP(c, hipSetDevice(c->device));
    return LPF_OK;
}

// `bytes` of host memory -> device memory `dst`, in stream order, WITHOUT waiting: the data is copied into the pinned ring
// (which an asynchronous copy may read from whenever it executes) and the copy is queued from there.  Only an upload larger
// than a quarter of the ring takes the blocking route: everything owed is launched, the stream drained, the copy made.
#define LPF_RING_BYTES (8u << 20)
int upload(lpf_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (bytes == 0) return LPF_OK;
    if (c->capturing) return fail(c, LPF_ERR_STATE, "a table upload cannot be captured into a graph: run the same shapes once before lpf_graph_begin");
    lpf_ctx::PinRing &R = c->ring;
    if (!R.base) {
        LPF_HIP(c, hipHostMalloc((void **)&R.base, LPF_RING_BYTES, hipHostMallocDefault));
        R.cap = LPF_RING_BYTES; R.head = 0;
        for (hipEvent_t &e : R.ev) LPF_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const size_t q = R.cap / 4, need = align256(bytes);
    if (need >= q) {
        int rc_ = sync_all(c);
        if (rc_) return rc_;
        LPF_HIP(c, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        ++c->stats[6];
        return LPF_OK;
    }
    // Invariant: head < cap, and head never rests on a quarter's end -- a piece that would fill its quarter exactly starts the
    // next one instead (">=": every `need` and q are multiples of 256, so exact fills are the common case, not the rare one; with
    // ">" the head walked to `cap` after 32768 small uploads and the next copy went past the ring).
    size_t cur = R.head / q;
    if (R.head - cur * q + need >= q) {                     // leave this quarter: it is reusable once what was queued from it has run
        LPF_HIP(c, hipEventRecord(R.ev[cur], c->stream));
        R.rec[cur] = true;
        cur = (cur + 1) & 3;
        R.head = cur * q;
        if (R.rec[cur]) {
            if (hipEventQuery(R.ev[cur]) != hipSuccess) { ++c->stats[0]; LPF_HIP(c, hipEventSynchronize(R.ev[cur])); }
            R.rec[cur] = false;
        }   // a full lap of uploads ago: long done
    }
    char *h = R.base + R.head;
    R.head += need;
    memcpy(h, src, bytes);
    ++c->stats[2];
    LPF_HIP(c, hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, c->stream));
    return LPF_OK;
}

// A table of n records -> buf, reserved here, through the pinned ring in pieces of LPF_TABLE_PIECE records: each under a quarter of the
// ring, so none takes upload()'s blocking route, whatever n is
#define LPF_TABLE_PIECE 32768
template <typename T> int upload_table(lpf_ctx *c, DevBuf &buf, const T *tab, size_t n)
{
    static_assert(sizeof(T) * LPF_TABLE_PIECE + 256 < LPF_RING_BYTES / 4, "a piece must stay under a quarter of the ring");
    int rc;
    if ((rc = reserve(c, buf, n * sizeof(T)))) return rc;
    for (size_t i = 0; i < n; i += LPF_TABLE_PIECE)
        if ((rc = upload(c, (T *)buf.p + i, tab + i, std::min(n - i, (size_t)LPF_TABLE_PIECE) * sizeof(T)))) return rc;
    return LPF_OK;
}

// How a batched call cuts its items (frames, images) into ranges of consecutive items: a range grows while it has fewer than
// most_items items -- what one launch takes -- and cost(first, count), the bytes it would stage, stays within LPF_STAGE_BUDGET; an item
// that needs more by itself is a range of its own.  The ranges are planned, and every buffer reserved for the largest of them
// (largest()), before the first launch, so no range waits for the one before it.
#define LPF_STAGE_BUDGET (256ull << 20)
// The budget, the most items of a range or launch (most: the product's limit) and the count lpf_lab_last_ranges reports: constants and
// nothing in the product, lpf_lab_set_range_limits' in a lab build
#ifdef LPF_LAB
static size_t stage_budget(const lpf_ctx *c) { return c->lab_budget > 0 ? (size_t)c->lab_budget : (size_t)LPF_STAGE_BUDGET; }
static size_t most_of(const lpf_ctx *c, size_t most) { return c->lab_max_items > 0 ? std::min(most, (size_t)c->lab_max_items) : most; }
static void note_ranges(lpf_ctx *c, size_t n) { c->lab_ranges = (int)n; }
#else
static constexpr size_t stage_budget(const lpf_ctx *) { return (size_t)LPF_STAGE_BUDGET; }
static constexpr size_t most_of(const lpf_ctx *, size_t most) { return most; }
static void note_ranges(lpf_ctx *, size_t) {}
#endif
template <typename Cost> std::vector<Span> plan_ranges(lpf_ctx *c, size_t items, size_t most_items, Cost &&cost)
{
    const size_t budget = stage_budget(c), most = most_of(c, most_items);
    std::vector<Span> ranges;
    for (size_t i0 = 0; i0 < items;) {
        size_t n = 1;
        while (i0 + n < items && n < most && cost(i0, n + 1) <= budget) ++n;
        ranges.push_back({i0, n});
        i0 += n;
    }
    note_ranges(c, ranges.size());
    return ranges;
}
template <typename Qty> size_t largest(const std::vector<Span> &ranges, Qty &&qty)
{
    size_t most = 0;
    for (const Span &r : ranges) most = std::max(most, (size_t)qty(r.first, r.count));
    return most;
}

// What a batched call begins with: a context, its device, no graph capture in progress (who: the call's name, as the refusal says it)
// and, where the call projects, a camera.
int enter(lpf_ctx *c, const char *who, bool need_camera)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (c->capturing) return fail(c, LPF_ERR_STATE, "%s cannot be captured into a graph (call it outside lpf_graph_begin ... lpf_graph_end)", who);
    if (need_camera && !c->have_camera) return fail(c, LPF_ERR_STATE, "lpf_set_camera has not been called");
    note_ranges(c, 0);
    return LPF_OK;
}

// The points [first, first + count) of a caller -> *dev: a device caller's, and no points, are lent; a host caller's are copied in stream
// order into buf -- reserved for `most` points, the largest range the call will ask for -- and *wait_owed is set: the call has to end
// with a host_wait, so that the caller may reuse its memory.
int host_points(lpf_ctx *c, DevBuf &buf, const float *pts, bool on_device, size_t first, size_t count, size_t most, const float4 **dev,
                bool *wait_owed)
{
    *dev = (const float4 *)pts + first;
    if (on_device || count == 0) return LPF_OK;
    int rc;
    if ((rc = reserve(c, buf, most * 16))) return rc;
    LPF_HIP(c, hipMemcpyAsync(buf.p, pts + 4 * first, count * 16, hipMemcpyHostToDevice, c->stream));
    *dev = (const float4 *)buf.p;
    *wait_owed = true;
    return LPF_OK;
}

// Offsets `name` [F + 1] of a call `who`: they start at 0 or above and do not decrease.
int check_offsets(lpf_ctx *c, const char *who, const char *name, const int32_t *off, int F)
{
    if (off[0] < 0) return fail(c, LPF_ERR_ARG, "%s: %s[0]=%d (offsets start at 0 or above)", who, name, off[0]);
    for (int f = 0; f < F; ++f)
        if (off[f + 1] < off[f]) return fail(c, LPF_ERR_ARG, "%s: %s decreases at frame %d", who, name, f);
    return LPF_OK;
}

// ---- what lpf_match_2d and lpf_assign_costs / lpf_assign_2d share on the host: a batch of frames of D x B pairs -------------------------
// The arrays and weights of a lpf_match2d_input (who: the call, as the refusals say it).  arrays: det_off and box_off are there to be
// read -- they are checked here, and dets / bbox2d / front against their totals.  with_min_iou: min_iou is in use and has to be finite.
int check_m2_input(lpf_ctx *c, const char *who, int F, const lpf_match2d_input *in, bool arrays, bool with_min_iou)
{
    int rc;
    if (arrays) {
        if ((rc = check_offsets(c, who, "det_off", in->det_off, F)) || (rc = check_offsets(c, who, "box_off", in->box_off, F))) return rc;
        const int Dtot = in->det_off[F], Btot = in->box_off[F];
        if ((Dtot > 0 && !in->dets) || (Btot > 0 && (!in->bbox2d || !in->front)))
            return fail(c, LPF_ERR_ARG, "%s: dets=%p bbox2d=%p front=%p with %d detections and %d boxes (dets is required with detections, bbox2d and front with boxes)",
                        who, in->dets, (const void *)in->bbox2d, (const void *)in->front, Dtot, Btot);
    }
    const bool weights = std::isfinite(in->w_iou) && std::isfinite(in->w_center) && std::isfinite(in->w_size);
    if (with_min_iou && !(weights && std::isfinite(in->min_iou)))
        return fail(c, LPF_ERR_ARG, "%s: min_iou=%g weights=%g %g %g must be finite", who, in->min_iou, in->w_iou, in->w_center, in->w_size);
    if (!weights) return fail(c, LPF_ERR_ARG, "%s: weights=%g %g %g must be finite", who, in->w_iou, in->w_center, in->w_size);
    return LPF_OK;
}

// The pair table of a batch and its ranges of consecutive frames (plan_ranges; bytes(t): what frame t adds to a range's staging and
// scratch), with the most detections, boxes, pairs and frames of any range: what the call's buffers are reserved for.
struct M2Range { size_t fa, nf, d0, nd, b0, nb, p0, np; int most_rows; };   // first frame and count; detections, boxes, pairs; the tallest frame
struct M2Plan { std::vector<LpfM2Frame> tab; std::vector<M2Range> ranges; size_t most_d = 0, most_b = 0, most_p = 0, most_f = 0; };
template <typename Bytes> M2Plan m2_plan(lpf_ctx *c, const int32_t *det_off, const int32_t *box_off, int F, size_t most_frames, Bytes &&bytes)
{
    M2Plan P;
    P.tab.resize((size_t)F + 1);                              // (one past the end: where the detections, boxes and pairs end)
    std::vector<size_t> cost((size_t)F + 1, 0);               // cost[f]: the bytes of the frames before f
    long long p = 0;
    for (int f = 0; f < F; ++f) {
        LpfM2Frame &t = P.tab[(size_t)f];
        t.d0 = det_off[f]; t.D = det_off[f + 1] - t.d0;
        t.b0 = box_off[f]; t.B = box_off[f + 1] - t.b0;
        t.p0 = p;
        p += (long long)t.D * t.B;
        cost[(size_t)f + 1] = cost[(size_t)f] + bytes(t);
    }
    P.tab[(size_t)F] = {det_off[F], 0, box_off[F], 0, p};
    for (const Span &r : plan_ranges(c, (size_t)F, most_frames, [&](size_t f, size_t n) { return cost[f + n] - cost[f]; })) {
        const LpfM2Frame &a = P.tab[r.first], &b = P.tab[r.first + r.count];
        M2Range R = {r.first, r.count, (size_t)a.d0, (size_t)(b.d0 - a.d0), (size_t)a.b0, (size_t)(b.b0 - a.b0), (size_t)a.p0, (size_t)(b.p0 - a.p0), 0};
        for (size_t f = R.fa; f < R.fa + R.nf; ++f) R.most_rows = std::max(R.most_rows, P.tab[f].D);
        P.most_d = std::max(P.most_d, R.nd); P.most_b = std::max(P.most_b, R.nb); P.most_p = std::max(P.most_p, R.np); P.most_f = std::max(P.most_f, R.nf);
        P.ranges.push_back(R);
    }
    return P;
}

// Every *_base of a range by one rule: a staged array begins at the range's first item, the caller's own at the batch's
template <typename T> T range_base(bool staged, T first) { return staged ? first : (T)0; }

// The box set in force, for a call `who` that tests the points of F frames against it: there must be one, set for F frames.
int boxes_in_force(lpf_ctx *c, const char *who, int F, lpf_ctx::BoxSet **BX)
{
    *BX = &c->boxes.in_force();
    if ((*BX)->F == 0) return fail(c, LPF_ERR_STATE, "%s: no boxes in force (lpf_set_boxes* comes first)", who);
    if ((*BX)->F != F) return fail(c, LPF_ERR_STATE, "boxes were set for %d frames, %s has %d", (*BX)->F, who, F);
    return LPF_OK;
}

// The frame table of such a call in HBM (buf): per frame its points and its boxes in BX.
int upload_batch_frames(lpf_ctx *c, DevBuf &buf, const int64_t *frame_off, int F, const lpf_ctx::BoxSet &BX)
{
    std::vector<LpfBatchFrame> tab((size_t)F);
    for (int f = 0; f < F; ++f) {
        LpfBatchFrame &t = tab[(size_t)f];
        t.pt_off = (long long)frame_off[f]; t.N = (int)(frame_off[f + 1] - frame_off[f]);
        t.box_off = BX.box_off[f]; t.B = BX.box_off[f + 1] - BX.box_off[f]; t.pad = 0;
    }
    return upload_table(c, buf, tab.data(), (size_t)F);
}

// The address a kernel may write for a host pointer that lies in page-locked, GPU-mapped memory (hipHostMalloc / lpf_host_alloc,
// hipHostRegister), or NULL for any other memory.  Asked every time: the answer for an address can change between calls.
void *device_alias_of_pinned(void *host)
{
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }    // (plain malloc memory: an error in some runtimes)
    // (hostPointer == host: the answer is about THIS address -- a pointer into the middle of an allocation is only taken when the runtime
    //  says so itself, never by assuming that its device alias lies at the same offset)
    return (at.type == hipMemoryTypeHost && at.hostPointer == host) ? at.devicePointer : nullptr;
}

// box parameters in the oracle's arithmetic (oracle/lpf_oracle.c: orc_oriented_inside) for lpf_points_in_boxes
void box_params(const double *c, int oriented, double *o)
{
    for (int i = 0; i < 16; ++i) o[i] = 0.0;
    if (oriented) {
        static const int other[3] = {1, 3, 4};
        o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
        bool ok = true;
        for (int a = 0; a < 3; ++a) {
            const double *p = c + 3 * other[a];
            const double v0 = p[0] - c[0], v1 = p[1] - c[1], v2 = p[2] - c[2];
            double w = v0 * v0; w = std::fma(v1, v1, w); w = std::fma(v2, v2, w);
            o[3 + 4 * a] = v0; o[4 + 4 * a] = v1; o[5 + 4 * a] = v2; o[6 + 4 * a] = w;
            if (!(w >= 1e-100 && w <= 1e100)) ok = false;      // also false for NaN; the range in which the kernel's
                                                               // division-free slab test is provably the quotient test (see lpf_oriented_inside)
        }
        o[15] = ok ? 1.0 : 0.0;            // 1: "0 <= d <= vv" decides the slab exactly (see kernel comment)
    } else {
        for (int k = 0; k < 3; ++k) {
            double a = c[k], b = c[k];
            for (int j = 1; j < 8; ++j) {
                const double w = c[3 * j + k];
                if (w < a) a = w;
                if (w > b) b = w;
            }
            o[k] = a; o[3 + k] = b;
        }
    }
}

int box_shape(lpf_ctx *c, lpf_ctx::BoxSet &B, const int32_t *box_off, int F, int oriented);

// The box set a lpf_set_boxes* call writes (lpf_ctx::Boxes::set_for_write; refused arguments leave the boxes in force as they are),
// then its shapes: per-frame records, grid offsets, buffers.  Nothing here waits for the GPU unless a buffer has to grow.
int box_layout(lpf_ctx *c, const int32_t *box_off, int F, int oriented, const char *who, lpf_ctx::BoxSet **out)
{
    if (F < 0 || (F > 0 && !box_off)) return fail(c, LPF_ERR_ARG, "%s: F=%d box_off=%p", who, F, (const void *)box_off);
    if (F > 0 && box_off[0] != 0) return fail(c, LPF_ERR_ARG, "%s: box_off[0] must be 0", who);
    for (int f = 0; f < F; ++f)
        if (box_off[f + 1] < box_off[f]) return fail(c, LPF_ERR_ARG, "%s: box_off not ascending at %d", who, f);
    if (!c->have_camera) return fail(c, LPF_ERR_STATE, "%s: lpf_set_camera must be called first (cam-0 boxes are filtered with its K, W, H)", who);
    int rc;
    bool owed;
    lpf_ctx::BoxSet *B = &c->boxes.set_for_write(c->pipe.fused, c->pipe.depth(), &owed);
    if (owed && (rc = flush_pending(c))) return rc;        // (still no host wait)
    if ((rc = box_shape(c, *B, box_off, F, oriented))) return rc;
    *out = B;
    return LPF_OK;
}

// a box set's shapes for F frames of box_off: per-frame records, grid offsets, buffers (the job that fills the tables comes later);
// the set holds no boxes until the last buffer is there
int box_shape(lpf_ctx *c, lpf_ctx::BoxSet &BS, const int32_t *box_off, int F, int oriented)
{
    int rc;
    lpf_ctx::BoxSet *B = &BS;
    B->begin();
    B->h_bframes.resize((size_t)F);
    B->cand_off.assign((size_t)F, 0);
    B->max_words = 1;
    size_t total = 0;
    for (int f = 0; f < F; ++f) {
        const int nb = box_off[f + 1] - box_off[f];
        B->h_bframes[f].box_off = box_off[f]; B->h_bframes[f].B = nb; B->h_bframes[f].cand_off = (long long)total;
        B->cand_off[f] = (long long)total;
        total += (size_t)LPF_GRID_WORDS * (size_t)((nb + 63) / 64);      // a ground grid per 64 boxes
        if ((nb + 63) / 64 > B->max_words) B->max_words = (nb + 63) / 64;
    }
    const int Btot = F ? box_off[F] : 0;
    const size_t nb = (size_t)(Btot ? Btot : 1);
    if ((rc = reserve(c, B->boxp, nb * 16 * sizeof(double)))) return rc;
    if ((rc = reserve(c, B->boxq, nb * 8 * sizeof(float)))) return rc;
    if ((rc = reserve(c, B->cand, (total ? total : 1) * 8))) return rc;
    if ((rc = reserve(c, B->corners, nb * 24 * sizeof(double)))) return rc;
    if ((rc = reserve(c, B->enabled, nb))) return rc;
    if (F > 1) {
        if ((rc = reserve(c, B->bframes, (size_t)F * sizeof(LpfBoxFrame)))) return rc;
        if (B->h_bframes_dev.size() != B->h_bframes.size() ||
            memcmp(B->h_bframes_dev.data(), B->h_bframes.data(), (size_t)F * sizeof(LpfBoxFrame)) != 0) {
            if ((rc = upload(c, B->bframes.p, B->h_bframes.data(), (size_t)F * sizeof(LpfBoxFrame)))) return rc;
            B->h_bframes_dev = B->h_bframes;
            ++c->generation;                                  // graphs captured for other box counts index these tables
        }
    }
    B->cand_words = total;
    B->shaped(box_off, F, oriented);
    return LPF_OK;
}

// The corners a set's job reads: the caller's own when they are lent device memory (on_device 2), else the set's copy of them, made
// here in stream order (an upload from host memory, a device copy).  nb boxes.
int stage_corners(lpf_ctx *c, lpf_ctx::BoxSet &B, const double *corners, int on_device, size_t nb, const double **src)
{
    int rc;
    *src = corners;
    if (on_device == 2) return LPF_OK;
    if ((rc = reserve(c, B.stage, nb * 192))) return rc;
    if (on_device) LPF_HIP(c, hipMemcpyAsync(B.stage.p, corners, nb * 192, hipMemcpyDeviceToDevice, c->stream));
    else if ((rc = upload(c, B.stage.p, corners, nb * 192))) return rc;
    *src = (const double *)B.stage.p;
    return LPF_OK;
}

// lpf_set_boxes_ex / lpf_set_boxes_cam0: corners (velodyne or cam-0 frame) -> the job that builds the set's tables.  The job is
// launched here when the caller wants results in host memory (then the call waits for them), in serial mode and inside a graph
// capture; a software-pipelined context leaves it to the next lpf_run*, in whose launch it rides.
int set_boxes_impl(lpf_ctx *c, const double *corners, int on_device, const int32_t *box_off, int F, int oriented, bool cam0, const double *Tcv,
                   int filter_visible, uint8_t *visible, double *corners_velo, double *bbox2d, int32_t *front, const char *who)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (on_device < 0 || on_device > 2) return fail(c, LPF_ERR_ARG, "%s: on_device=%d (0 host, 1 device, 2 device and lent)", who, on_device);
    if (F == 0) { c->boxes.in_force().clear(); return LPF_OK; }
    if (cam0 && !Tcv) return fail(c, LPF_ERR_ARG, "%s: T_cam_to_velo is NULL", who);
    if (box_off && F > 0 && box_off[F] > 0 && !corners) return fail(c, LPF_ERR_ARG, "%s: corners is NULL", who);
    int rc;
    lpf_ctx::BoxSet *B = nullptr;
    if ((rc = box_layout(c, box_off, F, oriented, who, &B))) return rc;
    const int Btot = box_off[F];
    if (Btot == 0) return LPF_OK;
    const size_t nb = (size_t)Btot;
    const double *src;
    if ((rc = stage_corners(c, *B, corners, on_device, nb, &src))) { B->clear(); return rc; }
    const bool host_out = !on_device && (visible || corners_velo || bbox2d || front);
    if (host_out && (rc = reserve(c, B->aux, nb * 36))) { B->clear(); return rc; }
    LpfBoxJob &J = B->new_job(src);
    J.filter_visible = filter_visible ? 1 : 0;
    if (cam0) {
        J.cam0 = 1;
        memcpy(J.Tcv, Tcv, sizeof J.Tcv);
        J.enabled_out = (uint8_t *)B->enabled.p;
        if (on_device) { J.visible = visible; J.corners_out = corners_velo; J.bbox2d = bbox2d; J.front = front; }
        else if (host_out) { J.bbox2d = (double *)B->aux.p; J.front = (int32_t *)((char *)B->aux.p + nb * 32); }
    }
    // The job waits for the next lpf_run* and rides in the launch of its streaming tiles (every mode: in order too the tables are
    // only read by the tail, one launch later) -- unless the caller wants results in host memory now.
    if (host_out && (rc = launch_box_job(c, *B))) return rc;
    if (host_out) {
        if (visible) LPF_HIP(c, hipMemcpyAsync(visible, B->enabled.p, nb, hipMemcpyDeviceToHost, c->stream));
        if (corners_velo) LPF_HIP(c, hipMemcpyAsync(corners_velo, B->corners.p, nb * 192, hipMemcpyDeviceToHost, c->stream));
        if (bbox2d) LPF_HIP(c, hipMemcpyAsync(bbox2d, B->aux.p, nb * 32, hipMemcpyDeviceToHost, c->stream));
        if (front) LPF_HIP(c, hipMemcpyAsync(front, (char *)B->aux.p + nb * 32, nb * 4, hipMemcpyDeviceToHost, c->stream));
        LPF_HIP(c, host_wait(c));       // the caller's host buffers are filled on return
    }
    return LPF_OK;
}

// What `iters` erosion iterations come to under the context's element (lpf_set_erosion_element): the 1 x 1 element is the identity, any
// number of iterations; a k x k element other than the 3 x 3 cross takes its own kernels (the _k ones)
struct Erosion { int iters; bool element; };
Erosion erosion(const lpf_ctx *c, int iters)
{
    if (c->erode_k == 1) iters = 0;
    return Erosion{iters, iters > 0 && c->erode_k != 3};
}

// `left` erosion iterations on the packed label image cur ([F][H][W] elements LT), one launch each, on stream ms: the cross, or
// (element) the context's k x k element.  Ping-pong with lb_, reserved here like every label image at 4 bytes per pixel; cur ends as
// the buffer that holds the result.  Every erosion of a packed image goes through here: the narrow label images (pack_masks,
// rle_label_image) and the wide passes' planes (wide_pack: F * LW images of uint32_t).
template <typename LT> int erode_packed_iters(lpf_ctx *c, LT *&cur, DevBuf &lb_, const int W, const int H, const int F, hipStream_t ms, int left, bool element)
{
    if (left <= 0) return LPF_OK;
    int rc;
    if ((rc = reserve(c, lb_, (size_t)F * H * W * 4))) return rc;
    const dim3 grid((W + LPF_TW - 1) / LPF_TW, (H + LPF_TH - 1) / LPF_TH, F);
    LT *other = (LT *)lb_.p;
    for (int it = 0; it < left; ++it) {
        if (element) hipLaunchKernelGGL((lpf_erode_packed_k<LT>), grid, dim3(LPF_BLOCK), 0, ms, cur, other, H, W, c->erode_r, c->erode_spans);
        else hipLaunchKernelGGL((lpf_erode_packed<LT>), grid, dim3(LPF_BLOCK), 0, ms, cur, other, H, W);
        LPF_HIP(c, hipGetLastError());
        LT *t = cur; cur = other; other = t;
    }
    return LPF_OK;
}

// masks [F][M][H][W] (uint8 under rule 0, or float under rule 1..3) -> label image with elements of `label_bytes`, on stream ms, into la
// (lb_ = erosion ping-pong): the context's camera size for the narrow calls (a scratch set's label_a / label_b), camera c's for
// lpf_run_cams
int pack_masks(lpf_ctx *c, DevBuf &la, DevBuf &lb_, const int W, const int H, hipStream_t ms, const void *masks, bool f32, int rule,
               int label_bytes, int F, int M, int erode_iters, void **result, const int4 *rects = nullptr)
{
    return with_label(label_bytes, [&](auto lt) -> int {
        typedef typename decltype(lt)::type LT;
        const size_t hw = (size_t)H * W;
        dim3 grid((W + LPF_TW - 1) / LPF_TW, (H + LPF_TH - 1) / LPF_TH, F);
        LT *cur = (LT *)la.p;
        int rc;
        if (M == 0) {
            LPF_HIP(c, hipMemsetAsync(cur, 0, (size_t)F * hw * sizeof(LT), ms));
        } else {
            // the k x k element of lpf_set_erosion_element: its own pack (first erosion fused, whatever the shape) and erosion kernel
            const Erosion E = erosion(c, erode_iters);
            int left = E.iters;
            const bool stream16 = !E.element && hw % 16 == 0 && ((uintptr_t)masks & 15) == 0;
            if (!stream16 && E.iters > 0) --left;          // (the tiled pack does the first erosion itself)
            with_rule(f32, rule, [&](auto kind) {
                typedef typename decltype(kind)::elem T;
                constexpr int RULE = decltype(kind)::rule;
                // (rectangles: only where set_masks_impl accepted them -- uint8 rule 0 / float rule 1, no erosion)
                const int4 *r = RULE <= 1 ? rects : nullptr;
                if (stream16) {
                    // streaming pack, 16 pixels per lane; erosion (if any) then runs on the packed image
                    const long long total16 = (long long)F * (long long)(hw / 16);
                    const unsigned nb = (unsigned)((total16 + LPF_BLOCK - 1) / LPF_BLOCK);
                    hipLaunchKernelGGL((lpf_pack16<T, RULE, LT>), dim3(nb), dim3(LPF_BLOCK), 0, ms, (const T *)masks, cur, M, (long long)hw, total16, r, W);
                } else if (E.element) {
                    hipLaunchKernelGGL((lpf_pack_erode_k<T, RULE, LT>), grid, dim3(LPF_BLOCK), 0, ms, (const T *)masks, cur, M, H, W, c->erode_r, c->erode_spans);
                } else {
                    hipLaunchKernelGGL((lpf_pack_erode<T, RULE, LT>), grid, dim3(LPF_BLOCK), 0, ms, (const T *)masks, cur, M, H, W, E.iters > 0 ? 1 : 0, r);
                }
            });
            LPF_HIP(c, hipGetLastError());
            if ((rc = erode_packed_iters(c, cur, lb_, W, H, F, ms, left, E.element))) return rc;
        }
        *result = cur;
        return LPF_OK;
    });
}

// the refusal of more masks per frame than a narrow run takes (lpf_set_masks_u8 / _f32 / _rle)
int too_many_masks(lpf_ctx *c, int M)
{
    return fail(c, LPF_ERR_ARG, "set_masks: M=%d masks per frame, a run takes at most LPF_MAX_MASKS = %d (one bit each in label_bits): run the frame "
                                "once per group of %d masks -- everything per point is the same in every pass (pipeline.run_frames does so)",
                M, LPF_MAX_MASKS, LPF_MAX_MASKS);
}

template <typename T>
int set_masks_impl(lpf_ctx *c, const T *masks, int F, int M, int mode, int erode_iters, int on_device)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (!c->have_camera) return fail(c, LPF_ERR_STATE, "lpf_set_camera must be called before masks (W, H)");
    if (M > LPF_MAX_MASKS) return too_many_masks(c, M);
    if (F < 0 || M < 0 || erode_iters < 0 || (F > 0 && M > 0 && !masks))
        return fail(c, LPF_ERR_ARG, "set_masks: F=%d M=%d erode_iters=%d masks=%p", F, M, erode_iters, (const void *)masks);
    // software-pipelined modes + device masks: the label images rotate with the scratch sets (the tiles of the previous run may
    // still have to read theirs); anything else uses set 0, with nothing owed
    const bool per_set = c->pipe.fused && on_device;
    int rc;
    if (!per_set && c->pipe.owes() && (rc = sync_all(c))) return rc;      // owed tiles read set 0's label image / the staging copy
    // (host masks in a pipelined mode: the pipeline has just been drained -- the staging copy is one -- and their label image goes to
    //  the set of the next run too, where a fused run looks for it, as lpf_set_label_image's does: in set 0 every run but the first after
    //  a mode switch was refused with "the masks were set for another scratch set")
    lpf_ctx::Masks &MK = c->masks;
    lpf_ctx::Scratch &S = c->sc[c->pipe.set_now()];
    // (masks a pipelined lpf_set_masks_* left unpacked stay on record until this call has its buffers -- so also when it is for no
    //  frames: the next run packs them.  Kept as it was)
    MK.begin(c->pipe.set_now());
    if (F == 0) return LPF_OK;
    const size_t hw = (size_t)c->H * c->W;
    if ((rc = reserve(c, S.label_a, (size_t)F * hw * 4))) return rc;
    const T *d_masks = masks;
    if (M > 0 && !on_device) {
        const size_t bytes = (size_t)F * M * hw * sizeof(T);
        if ((rc = reserve(c, c->mask_stage, bytes))) return rc;
        LPF_HIP(c, hipMemcpyAsync(c->mask_stage.p, masks, bytes, hipMemcpyHostToDevice, c->stream));
        d_masks = (const T *)c->mask_stage.p;
    }
    const int lb = (M <= 8) ? 1 : (M <= 16) ? 2 : 4;
    // rectangles given for these masks (lpf_set_mask_rects): used where uint8 masks are packed as they are; consumed either way
    const int4 *rects = (((sizeof(T) == 1 && mode == 0) || (sizeof(T) == 4 && mode == 1)) && erode_iters == 0 && c->rects_F == F && c->rects_M == M &&
                         c->W >= 16) ? c->rects_pending : nullptr;         // (W >= 16: a group of 16 pixels of the pack spans at most two rows)
    c->rects_pending = nullptr;
    MK.forget_unpacked();
    const bool lent_pipelined = per_set && on_device == 2, kept_serial = !c->pipe.fused && on_device != 1;
    if (M > 0 && erode_iters == 0 && (lent_pipelined || kept_serial)) {
        // nothing to erode, and the masks stay where they are (lent by the caller, or -- serial mode -- our staging buffer): packing
        // is left to the next lpf_run* (see lpf_ctx::Unpacked) -- a launch of sparse frames does without it
        lpf_ctx::Unpacked &U = MK.unpacked;                // (forgotten above: every field is at its default)
        U.valid = true; U.pipelined = lent_pipelined; U.masks = d_masks; U.f32 = sizeof(T) == 4; U.rule = mode; U.F = F; U.M = M;
        U.rects = rects; U.label = S.label_a.p;
        U.can_ride = lent_pipelined && c->pipe.defer && sizeof(T) == 1 && hw % 16 == 0 && ((uintptr_t)d_masks & 15) == 0;
        if (!on_device) LPF_HIP(c, host_wait(c));         // the host buffer may be reused by the caller
        MK.left_unpacked(lent_pipelined ? S.label_a.p : nullptr, lb);
        return LPF_OK;
    }
    void *cur = nullptr;
    if ((rc = pack_masks(c, S.label_a, S.label_b, c->W, c->H, c->stream, d_masks, sizeof(T) == 4, mode, lb, F, M, erode_iters, &cur, rects))) return rc;
    if (!on_device) LPF_HIP(c, host_wait(c));   // the host buffer may be reused by the caller
    MK.packed(F, M, cur, lb);
    return LPF_OK;
}

// masks that are set but not packed (lpf_ctx::Unpacked) -> packed now, by a launch of their own, into the label image of their scratch
// set (set 0 in serial mode).  The frames and masks in force stay as they are: after lpf_set_label_image they are that image's
int pack_unpacked(lpf_ctx *c)
{
    lpf_ctx::Masks &MK = c->masks;
    const lpf_ctx::Unpacked &U = MK.unpacked;
    if (!U.valid) return LPF_OK;
    lpf_ctx::Scratch &S = c->sc[MK.set];
    void *cur = nullptr;
    int rc = pack_masks(c, S.label_a, S.label_b, c->W, c->H, c->stream, U.masks, U.f32, U.rule, MK.bytes, U.F, U.M, 0, &cur, U.rects);
    if (rc) return rc;
    MK.packed(MK.F, MK.M, cur, MK.bytes);
    MK.forget_unpacked();
    return LPF_OK;
}

// Where the tiles of a run of lpf_run_batch get their label bits: a run of M masks (0: none) on a context whose masks may still be
// unpacked (lpf_ctx::Unpacked); fused: one launch per run, the tail rides in the next; small: the small geometry; sparse_frames: the
// run has at most half as many points as its images have pixels.  Masks that this run neither reads directly nor lets ride are packed
// here, now (same stream, ahead of the tiles).
//   Unpacked masks are read directly only by the kind of run they were left for: those a pipelined lpf_set_masks_* lent, by a fused
// run -- a host-memory run or one with host points packs them now; those a serial call left are never met by a fused run
// (lpf_set_pipelined packs them on the switch).
//   A small fused launch reads lent masks directly, a large one in mode 4 carries their pack, anything else (mode 2, float masks, a
// host-memory run) packs them now
// (directly: M gathers per valid point against M reads per pixel for the pack -- it pays while a frame has fewer points than
//  half its image has pixels: a real scan, 110 k points on 530 k pixels, 29.9 -> 24.9 us per 20-frame batch in a pipelined
//  stream; a synthetic 2 M-point cloud is better off with the pack riding, 21.8 vs 24.2 us)
// ... and with the masks' rectangles (lpf_set_mask_rects) a launch of sparse frames of ANY size reads the masks inside them: no
// pack, no label image (146 real frames per step: 176 -> 134 us).  Dense frames keep the pack: with 2 M points on 530 k pixels and
// rectangles that cover a good part of the image every row meets a rectangle, and the exact test of such a row is a dependent round
// trip (one 2 M-point cloud with 8 disk masks, tiles 18.5 -> 21 us, pipelined stream 21.4 -> 25.4 us per cloud).
// Small launches stay with the tiles that read all M mask bytes of a valid point (LpfDirect) and gate them by the rectangles: the
// candidate grid would be one more kernel in front of a launch that is as long as its chain (a single real frame in order 18.8 vs
// 23.0 us; pipelined 11.1 vs 10.2, 4 frames 21.1 vs 21.4, 20 frames 35.0 vs 36.6).
//   Masks left unpacked in serial mode: a small serial launch reads them directly, anything else packs them now.
int plan_tile_source(lpf_ctx *c, bool fused, bool small, bool sparse_frames, int M, TileSource &src)
{
    src = TileSource();
    int rc;
    const lpf_ctx::Masks &MK = c->masks;
    const lpf_ctx::Unpacked &U = MK.unpacked;
    const bool readable = U.valid && U.pipelined == fused && M > 0 && sparse_frames;
    if (readable && !small && U.rects && ((!U.f32 && U.rule == 0) || (U.f32 && U.rule == 1))) src.kind = TileSource::DIRECT_RECT;
    else if (readable && small) src.kind = TileSource::DIRECT;
    else {
        src.ride_pack = U.valid && U.pipelined && fused && U.can_ride && M > 0;
        if (!src.ride_pack && (rc = pack_unpacked(c))) return rc;
        if (M > 0) src.kind = TileSource::PACKED;
    }
    // The label image lives in the scratch set that was current when the masks were set.  A pipelined run must find it in its
    // own set (the sets rotate: masks are set before every run); any other run has nothing owed and reads it where it is.
    if (M > 0 && fused && MK.set != c->pipe.run_set(fused))
        return fail(c, LPF_ERR_STATE, "the masks were set for another scratch set: in the pipelined modes the label images rotate with the scratch sets -- call lpf_set_masks_* before every lpf_run* (and after switching modes)");
    if (src.reads_masks()) {
        src.f32 = U.f32; src.rule = U.rule; src.img = U.masks;
        src.rects = U.rects;                               // (the rectangles also gate the tiles that read all M mask bytes: small sparse launches)
    } else if (M > 0) {
        src.img = MK.img;
    }
    if (M > 0 && !src.img) return fail(c, LPF_ERR_STATE, "no masks for this run's scratch set: in the pipelined modes the label images rotate with the scratch sets -- call lpf_set_masks_* before every lpf_run* (and after switching modes)");
    src.label_bytes = (M > 0) ? MK.bytes : 4;
    return LPF_OK;
}

// ---- run-length masks: the walk and the staging that lpf_set_masks_rle and the wide / multi-camera passes share --------------------

// The walk of a lpf_rle_masks for an image of hw pixels: every check of include/lpf.h, in 64 bits, and the emission of the decode's work
// units {run, first pixel} (lpf_rle.hip.h) into `units`.  Nothing is enqueued.  who: the messages' prefix -- "lpf_set_masks_rle", or a
// pass's "run_wide" / "run_cams_wide: camera 1"
int rle_walk(lpf_ctx *c, const char *who, const lpf_rle_masks *in, long long hw, std::vector<int2> &units, long long *Rtot_out)
{
    const int F = in->F, M = in->M;
    units.clear();
    *Rtot_out = 0;
    if (F < 0 || M < 0 || in->erode_iters < 0 || in->reserved != 0)
        return fail(c, LPF_ERR_ARG, "%s: F=%d M=%d erode_iters=%d reserved=%d", who, F, M, in->erode_iters, in->reserved);
    const long long FM = (long long)F * M;
    if (FM > 0x7fffffffll) return fail(c, LPF_ERR_ARG, "%s: F * M = %lld masks (at most 2^31 - 1 in one call)", who, FM);
    if (FM == 0) return LPF_OK;
    const int64_t *off = in->run_off;
    if (!off) return fail(c, LPF_ERR_ARG, "%s: run_off=NULL with F=%d M=%d", who, F, M);
    if (off[0] != 0) return fail(c, LPF_ERR_ARG, "%s: run_off[0]=%lld (must be 0)", who, (long long)off[0]);
    for (long long k = 0; k < FM; ++k)
        if (off[k + 1] < off[k])
            return fail(c, LPF_ERR_ARG, "%s: run_off decreases at frame %lld mask %lld (%lld after %lld)", who, k / M, k % M,
                        (long long)off[k + 1], (long long)off[k]);
    const long long Rtot = off[FM];
    if (Rtot > 0x7fffffffll) return fail(c, LPF_ERR_ARG, "%s: %lld runs (at most 2^31 - 1 in one call)", who, Rtot);
    if (Rtot > 0 && !in->runs) return fail(c, LPF_ERR_ARG, "%s: runs=NULL with %lld runs", who, Rtot);
    for (long long k = 0; k < FM; ++k)
        for (long long r = off[k]; r < off[k + 1]; ++r) {
            const long long start = in->runs[2 * r], length = in->runs[2 * r + 1];
            if (start < 0 || length < 0 || start + length > hw)
                return fail(c, LPF_ERR_ARG, "%s: frame %lld mask %lld run %lld: start=%lld length=%lld (0 <= start, 0 <= length, "
                                            "start + length <= W*H = %lld)", who, k / M, k % M, r - off[k], start, length, hw);
            for (long long p = start; p < start + length; p += LPF_RLE_CHUNK) units.push_back(int2{(int)r, (int)p});
            if (units.size() > LPF_RLE_MAX_UNITS)
                return fail(c, LPF_ERR_ARG, "%s: the runs cover more than 2^24 chunks of %d pixels (frame %lld mask %lld run %lld): "
                                            "set fewer frames per call", who, LPF_RLE_CHUNK, k / M, k % M, r - off[k]);
        }
    *Rtot_out = Rtot;
    return LPF_OK;
}

// [runs | units | run_off] of a walked lpf_rle_masks with units (rle_walk), copied into `stage` in stream order -> the decode's job for
// an image of hw pixels, and its grid.  The caller owes a host_wait before `in`'s arrays and `units` may change
int rle_stage_tables(lpf_ctx *c, DevBuf &stage, const lpf_rle_masks *in, const std::vector<int2> &units, long long Rtot, long long hw,
                     LpfRleJob &J, unsigned *nblocks)
{
    const long long FM = (long long)in->F * in->M;
    const size_t b_runs = align256((size_t)Rtot * sizeof(int2)), b_units = align256(units.size() * sizeof(int2)), b_off = (size_t)(FM + 1) * 8;
    int rc;
    if ((rc = reserve(c, stage, b_runs + b_units + b_off))) return rc;
    char *d = (char *)stage.p;
    LPF_HIP(c, hipMemcpyAsync(d, in->runs, (size_t)Rtot * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    LPF_HIP(c, hipMemcpyAsync(d + b_runs, units.data(), units.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));
    LPF_HIP(c, hipMemcpyAsync(d + b_runs + b_units, in->run_off, b_off, hipMemcpyHostToDevice, c->stream));
    J.runs = (const int2 *)d; J.units = (const int2 *)(d + b_runs); J.run_off = (const long long *)(d + b_runs + b_units);
    J.hw = hw; J.n_units = (int)units.size(); J.M = in->M; J.FM = (int)FM;
    *nblocks = (unsigned)((units.size() + LPF_RLE_BLOCK / 64 - 1) / (LPF_RLE_BLOCK / 64));
    return LPF_OK;
}

// The narrow label image [F][H][W] of `label_bytes` per pixel from walked run-length masks R (R.in not NULL): zero, decode
// (lpf_rle_decode), then every erosion iteration on the packed image -- into la (lb_ = erosion ping-pong), the tables staged in `stage`.
// *result: the buffer that holds the image.  *staged is set once copies from the caller's arrays and R.units are queued: the caller owes
// the host wait.  For lpf_set_masks_rle (a scratch set's label image) and lpf_run_cams (a camera's)
int rle_label_image(lpf_ctx *c, DevBuf &la, DevBuf &lb_, DevBuf &stage, const lpf_ctx::RleIn &R, const int W, const int H, int label_bytes,
                    void **result, bool *staged)
{
    const int F = R.in->F;
    const size_t hw = (size_t)W * H;
    int rc;
    // 4 bytes per pixel whatever the element: the decode's 32-bit atomics on the last, partial word of an image of 1- or 2-byte
    // elements stay inside the allocation (lpf_rle.hip.h)
    if ((rc = reserve(c, la, (size_t)F * hw * 4))) return rc;
    LPF_HIP(c, hipMemsetAsync(la.p, 0, (size_t)F * hw * label_bytes, c->stream));
    *result = la.p;
    if (R.units.empty()) return LPF_OK;                    // (the image is zero, and erosion keeps it so)
    LpfRleJob J;
    unsigned nb = 0;
    if ((rc = rle_stage_tables(c, stage, R.in, R.units, R.Rtot, (long long)hw, J, &nb))) return rc;
    *staged = true;
    const Erosion E = erosion(c, R.in->erode_iters);
    return with_label(label_bytes, [&](auto lt) -> int {
        typedef typename decltype(lt)::type LT;
        hipLaunchKernelGGL((lpf_rle_decode<LT>), dim3(nb), dim3(LPF_RLE_BLOCK), 0, c->stream, J, (uint32_t *)la.p);
        LPF_HIP(c, hipGetLastError());
        LT *img = (LT *)la.p;
        const int rc_ = erode_packed_iters(c, img, lb_, W, H, F, c->stream, E.iters, E.element);
        *result = img;
        return rc_;
    });
}

// The wide passes' label planes [F][LW][Himg][Wimg] (wide_pack) from walked run-length masks R (R.in not NULL: its F frames, M masks,
// erosion), in D's planes_a / planes_b, *planes = the buffer that holds the result: zero ALL the planes (the bits above M of a frame's
// last word stay zero, as the dense pack leaves them), OR the runs in (lpf_rle_decode_wide), then every erosion iteration.  No dense
// mask is staged.  *host_in is set once copies from the caller's arrays and R.units are queued
int wide_pack_runs(lpf_ctx *c, lpf_ctx::Wide &D, const lpf_ctx::RleIn &R, int Wimg, int Himg, const uint32_t **planes, bool *host_in)
{
    int rc;
    const int F = R.in->F, LW = (R.in->M + 31) / 32;
    const size_t hw = (size_t)Wimg * Himg;
    if ((rc = reserve(c, D.planes_a, (size_t)F * LW * hw * 4))) return rc;
    uint32_t *cur = (uint32_t *)D.planes_a.p;
    LPF_HIP(c, hipMemsetAsync(cur, 0, (size_t)F * LW * hw * 4, c->stream));
    if (!R.units.empty()) {                               // (no units: the planes are zero, and erosion keeps them so)
        LpfRleJob J;
        unsigned nb = 0;
        if ((rc = rle_stage_tables(c, D.rle, R.in, R.units, R.Rtot, (long long)hw, J, &nb))) return rc;
        *host_in = true;
        hipLaunchKernelGGL(lpf_rle_decode_wide, dim3(nb), dim3(LPF_RLE_BLOCK), 0, c->stream, J, LW, cur);
        LPF_HIP(c, hipGetLastError());
        const Erosion E = erosion(c, R.in->erode_iters);
        if ((rc = erode_packed_iters(c, cur, D.planes_b, Wimg, Himg, F * LW, c->stream, E.iters, E.element))) return rc;
    }
    *planes = cur;
    return LPF_OK;
}

// ---- instance-ID maps (lpf_id_masks, include/lpf.h): the checks, the staging and the decodes of lpf_set_masks_ids / lpf_run_wide_ids ----

template <typename Fn> auto with_id(int id_bytes, Fn &&fn)
{
    if (id_bytes == 2) return fn(TypeTag<uint16_t>());
    return fn(TypeTag<int32_t>());
}

// blocks per frame of the ID-map decodes (lpf_ids.hip.h) for images of hw pixels: one thread per 16-byte group of IDs, hw / PER groups
// at the most whatever the frame's alignment; at least one block, which also takes the frame's head and tail
size_t ids_blocks(size_t hw, int id_bytes)
{
    const size_t nvec = hw / (size_t)(16 / id_bytes);
    return std::max<size_t>(1, (nvec + LPF_IDS_BLOCK - 1) / LPF_IDS_BLOCK);
}

// Every check of a lpf_id_masks (not NULL, its M within the call's limit) for images of hw pixels: each refusal names its field.  Nothing
// behind the two pointers is read -- any map and any table are valid input -- and nothing is enqueued.  who: the messages' prefix
int check_ids(lpf_ctx *c, const char *who, const lpf_id_masks *in, size_t hw)
{
    if (in->F < 0) return fail(c, LPF_ERR_ARG, "%s: F=%d (must be >= 0)", who, in->F);
    if (in->M < 0) return fail(c, LPF_ERR_ARG, "%s: M=%d (must be >= 0)", who, in->M);
    if (in->erode_iters < 0) return fail(c, LPF_ERR_ARG, "%s: erode_iters=%d (must be >= 0)", who, in->erode_iters);
    if (in->id_bytes != 2 && in->id_bytes != 4) return fail(c, LPF_ERR_ARG, "%s: id_bytes=%d (2: uint16 IDs, 4: int32 IDs)", who, in->id_bytes);
    if (in->on_device != 0 && in->on_device != 1)
        return fail(c, LPF_ERR_ARG, "%s: on_device=%d (0: ids in host memory, 1: device memory)", who, in->on_device);
    if (in->reserved != 0) return fail(c, LPF_ERR_ARG, "%s: reserved=%d (must be 0)", who, in->reserved);
    const long long FM = (long long)in->F * in->M;
    if (FM > 0x7fffffffll) return fail(c, LPF_ERR_ARG, "%s: F * M = %lld table entries (at most 2^31 - 1 in one call)", who, FM);
    if (in->F > 0 && !in->ids) return fail(c, LPF_ERR_ARG, "%s: ids=NULL with F=%d", who, in->F);
    if (FM > 0 && !in->sel) return fail(c, LPF_ERR_ARG, "%s: sel=NULL with F=%d M=%d", who, in->F, in->M);
    if ((unsigned long long)in->F * ids_blocks(hw, in->id_bytes) > 0x7fffffffull)
        return fail(c, LPF_ERR_ARG, "%s: F=%d frames of %zu pixels are more blocks than one launch takes (2^31 - 1): set fewer frames per call",
                    who, in->F, hw);
    return LPF_OK;
}

// [sel | host ids] of a checked lpf_id_masks (F * M > 0) for images of hw pixels -> `stage`, in stream order; *sel, *ids: what the decode
// reads.  sel goes through the pinned upload ring: it is copied when this returns, with no wait on the stream.  Host ids are copied from
// the caller's memory and *host_in is set -- the caller owes a host_wait before it returns; device ids are read where they are
int ids_stage_tables(lpf_ctx *c, DevBuf &stage, const lpf_id_masks *in, size_t hw, const int32_t **sel, const void **ids, bool *host_in)
{
    const size_t n_sel = (size_t)in->F * in->M * sizeof(int32_t), b_sel = align256(n_sel);
    const size_t b_ids = in->on_device ? 0 : (size_t)in->F * hw * in->id_bytes;
    int rc;
    if ((rc = reserve(c, stage, b_sel + b_ids))) return rc;
    if ((rc = upload(c, stage.p, in->sel, n_sel))) return rc;
    *sel = (const int32_t *)stage.p;
    *ids = in->ids;
    if (!in->on_device) {
        LPF_HIP(c, hipMemcpyAsync((char *)stage.p + b_sel, in->ids, b_ids, hipMemcpyHostToDevice, c->stream));
        *ids = (char *)stage.p + b_sel;
        *host_in = true;
    }
    return LPF_OK;
}

// The narrow label image [F][H][W] of `label_bytes` per pixel from a checked lpf_id_masks: ONE launch of lpf_ids_label writes every
// element (no memset in front), then every erosion iteration runs on the packed image -- into la (lb_ = erosion ping-pong), the tables
// staged in `stage`.  M = 0: the image is zeroed, nothing is launched.  *result: the buffer that holds the image
int ids_label_image(lpf_ctx *c, DevBuf &la, DevBuf &lb_, DevBuf &stage, const lpf_id_masks *in, const int W, const int H, int label_bytes,
                    void **result, bool *host_in)
{
    const int F = in->F, M = in->M;
    const size_t hw = (size_t)W * H;
    int rc;
    if ((rc = reserve(c, la, (size_t)F * hw * 4))) return rc;        // (4 bytes per pixel, as every label image is reserved)
    *result = la.p;
    if (M == 0) {
        LPF_HIP(c, hipMemsetAsync(la.p, 0, (size_t)F * hw * label_bytes, c->stream));
        return LPF_OK;
    }
    const int32_t *sel = nullptr;
    const void *ids = nullptr;
    if ((rc = ids_stage_tables(c, stage, in, hw, &sel, &ids, host_in))) return rc;
    const unsigned nblk = (unsigned)ids_blocks(hw, in->id_bytes);
    const Erosion E = erosion(c, in->erode_iters);
    return with_id(in->id_bytes, [&](auto it) -> int {
        typedef typename decltype(it)::type IT;
        return with_label(label_bytes, [&](auto lt) -> int {
            typedef typename decltype(lt)::type LT;
            hipLaunchKernelGGL((lpf_ids_label<IT, LT>), dim3(nblk * (unsigned)F), dim3(LPF_IDS_BLOCK), 0, c->stream, (const IT *)ids, sel,
                               (LT *)la.p, (long long)hw, M, nblk);
            LPF_HIP(c, hipGetLastError());
            LT *img = (LT *)la.p;
            const int rc_ = erode_packed_iters(c, img, lb_, W, H, F, c->stream, E.iters, E.element);
            *result = img;
            return rc_;
        });
    });
}

// The wide passes' label planes [F][LW][Himg][Wimg] (wide_pack) from a checked lpf_id_masks (M > 0), in D's planes_a / planes_b,
// *planes = the buffer that holds the result: ONE launch of lpf_ids_planes writes all F * LW * Himg * Wimg words (no memset in front;
// the bits at or above M are zero), then every erosion iteration.  No dense mask is staged
int wide_pack_ids(lpf_ctx *c, lpf_ctx::Wide &D, const lpf_id_masks *in, int Wimg, int Himg, const uint32_t **planes, bool *host_in)
{
    int rc;
    const int F = in->F, M = in->M, LW = (M + 31) / 32;
    const size_t hw = (size_t)Wimg * Himg;
    if ((rc = reserve(c, D.planes_a, (size_t)F * LW * hw * 4))) return rc;
    uint32_t *cur = (uint32_t *)D.planes_a.p;
    const int32_t *sel = nullptr;
    const void *ids = nullptr;
    if ((rc = ids_stage_tables(c, D.ids, in, hw, &sel, &ids, host_in))) return rc;
    const unsigned nblk = (unsigned)ids_blocks(hw, in->id_bytes);
    with_id(in->id_bytes, [&](auto it) {
        typedef typename decltype(it)::type IT;
        hipLaunchKernelGGL((lpf_ids_planes<IT>), dim3(nblk * (unsigned)F), dim3(LPF_IDS_BLOCK), 0, c->stream, (const IT *)ids, sel, cur,
                           (long long)hw, M, LW, nblk);
    });
    LPF_HIP(c, hipGetLastError());
    const Erosion E = erosion(c, in->erode_iters);
    if ((rc = erode_packed_iters(c, cur, D.planes_b, Wimg, Himg, F * LW, c->stream, E.iters, E.element))) return rc;
    *planes = cur;
    return LPF_OK;
}

// The frames [f0, f0 + fc) of a walked batch A (A.in->M > 0): rle_walk emits the units in run order, so the range's runs and units are
// contiguous pieces of A's.  rle_units_before: the units of the runs before run r, i.e. the first unit of r (or of the next run that has one)
size_t rle_units_before(const lpf_ctx::RleIn &A, long long r)
{
    return (size_t)(std::lower_bound(A.units.begin(), A.units.end(), r, [](const int2 &u, long long run) { return (long long)u.x < run; }) -
                    A.units.begin());
}
// ... the bytes rle_stage_tables stages for that range
size_t rle_slice_bytes(const lpf_ctx::RleIn &A, size_t f0, size_t fc)
{
    const size_t M = (size_t)A.in->M;
    const long long r0 = A.in->run_off[f0 * M], r1 = A.in->run_off[(f0 + fc) * M];
    return align256((size_t)(r1 - r0) * sizeof(int2)) + align256((rle_units_before(A, r1) - rle_units_before(A, r0)) * sizeof(int2)) +
           (fc * M + 1) * 8;
}
// ... and the range as a batch of its own in S (lpf_ctx::RleSlice): what wide_pack_runs takes as its checked input
void rle_slice(const lpf_ctx::RleIn &A, size_t f0, size_t fc, lpf_ctx::RleSlice &S)
{
    const size_t M = (size_t)A.in->M;
    const int64_t *off = A.in->run_off + f0 * M;
    const long long r0 = off[0], r1 = off[fc * M];
    S.off.resize(fc * M + 1);
    for (size_t k = 0; k <= fc * M; ++k) S.off[k] = off[k] - r0;
    const size_t u0 = rle_units_before(A, r0), u1 = rle_units_before(A, r1);
    S.R.units.assign(A.units.begin() + (ptrdiff_t)u0, A.units.begin() + (ptrdiff_t)u1);
    for (int2 &u : S.R.units) u.x -= (int)r0;
    S.sub = *A.in;
    S.sub.F = (int32_t)fc;
    S.sub.runs = r1 > r0 ? A.in->runs + 2 * r0 : nullptr;
    S.sub.run_off = S.off.data();
    S.R.in = &S.sub;
    S.R.Rtot = r1 - r0;
}

// The run-length masks of ONE call, walked into rle_in[0] before anything is enqueued (lpf_set_masks_rle; lpf_depth_maps_rle and
// lpf_first_match_rle, whose batch goes through in ranges of frames: what a range's tables cost, for plan_ranges; the largest range's
// buffers and every range's slice, lpf_ctx::RleSlice; the pack of range k).  By whatever way the call returns, errors included, nothing
// of the context points into the caller's arrays afterwards -- on the success path after the call's host wait: the queued copies
// read them.  Without a walk, or with M = 0, active() is false and bytes() is 0
struct RleCall {
    lpf_ctx *c;
    lpf_ctx::RleIn &A;
    int W = 0, H = 0;                                     // the masks' image
    explicit RleCall(lpf_ctx *c_) : c(c_), A(c_->rle_in[0]) { A.in = nullptr; }     // (whatever an earlier pass left there)
    RleCall(const RleCall &) = delete;
    ~RleCall() { c->rle_slices.clear(); A.in = nullptr; }
    bool active() const { return A.in && A.in->M > 0; }
    int walk(const char *who, const lpf_rle_masks *rle, int W_, int H_)
    {
        W = W_; H = H_;
        const int rc = rle_walk(c, who, rle, (long long)W * H, A.units, &A.Rtot);
        if (!rc) A.in = rle;
        return rc;
    }
    size_t bytes(size_t f0, size_t n) const { return active() ? rle_slice_bytes(A, f0, n) : 0; }
    // D's planes for the range of most frames (both sets with erosion: decoded planes are eroded from the first iteration on) and its
    // run tables for the range that stages most; every range's slice of the runs
    int reserve_ranges(lpf_ctx::Wide &D, const std::vector<Span> &ranges)
    {
        int rc;
        const size_t planes = largest(ranges, [](size_t, size_t n) { return n; }) * (size_t)((A.in->M + 31) / 32) * W * H * 4;
        if ((rc = reserve(c, D.planes_a, planes))) return rc;
        if (A.in->erode_iters > 0 && (rc = reserve(c, D.planes_b, planes))) return rc;
        if ((rc = reserve(c, D.rle, largest(ranges, [&](size_t f0, size_t n) { return bytes(f0, n); })))) return rc;
        c->rle_slices.resize(ranges.size());
        for (size_t k = 0; k < ranges.size(); ++k) rle_slice(A, ranges[k].first, ranges[k].count, c->rle_slices[k]);
        return LPF_OK;
    }
    // range k's planes: zeroed, its own runs decoded, every erosion iteration (wide_pack_runs on its slice)
    int pack(lpf_ctx::Wide &D, size_t k, const uint32_t **planes, bool *host_in) { return wide_pack_runs(c, D, c->rle_slices[k].R, W, H, planes, host_in); }
};

// What lpf_set_masks_rle and lpf_set_masks_ids do once their own checks have passed, for F frames of M <= LPF_MAX_MASKS masks: the
// state transitions of set_masks_impl with host masks -- drain what a pipelined context owes (not per scratch set), the label image of
// the set the next run reads -- with the form's decode in place of copy + pack.  Always packed at the call.  build(S, label_bytes, &cur,
// &host_in): the form's label image in S.label_a / S.label_b, *cur the buffer that holds it; *host_in: copies from the caller's memory
// were queued, so the call waits before it returns (the caller's arrays may be reused).  A pending lpf_set_mask_rects hint is consumed
// (neither runs nor a map need one) and unpacked masks are forgotten before the image is reserved.
template <typename Build> int set_masks_compact(lpf_ctx *c, int F, int M, Build &&build)
{
    int rc;
    if (c->pipe.owes() && (rc = sync_all(c))) return rc;
    lpf_ctx::Masks &MK = c->masks;
    lpf_ctx::Scratch &S = c->sc[c->pipe.set_now()];
    MK.begin(c->pipe.set_now());
    if (F == 0) return LPF_OK;
    const int lb = (M <= 8) ? 1 : (M <= 16) ? 2 : 4;
    c->rects_pending = nullptr;
    MK.forget_unpacked();
    void *cur = nullptr;
    bool host_in = false;
    if ((rc = build(S, lb, &cur, &host_in))) return rc;
    if (host_in) LPF_HIP(c, host_wait(c));
    MK.packed(F, M, cur, lb);
    return LPF_OK;
}

// ---- setup the run paths share ---------------------------------------------------------------------------------------------------

// frame_off[0..F] (not NULL, F > 0: the caller's checks) starts at 0 and has frames of 0 .. 0x7fffffff - slack points; pts is given if
// there are points.  who: the messages' prefix
int check_frames(lpf_ctx *c, const char *who, const float *pts, const int64_t *frame_off, int F, int64_t slack)
{
    if (frame_off[0] != 0) return fail(c, LPF_ERR_ARG, "%s: frame_off[0] must be 0", who);
    for (int f = 0; f < F; ++f) {
        const int64_t n = frame_off[f + 1] - frame_off[f];
        if (n < 0 || n > 0x7fffffffll - slack) return fail(c, LPF_ERR_ARG, "%s: frame %d has %lld points", who, f, (long long)n);
    }
    if (frame_off[F] > 0 && !pts) return fail(c, LPF_ERR_ARG, "%s: pts is NULL", who);
    return LPF_OK;
}

// a lpf_wide_input: 0 .. max_M masks per frame ("... M=<M> masks per frame, <takes> = <max_M><more>"), its form (f32: LPF_MASKS_U8 /
// _F32 / _RLE and nothing else; the run-length form only where the call takes it -- takes_rle -- and then in host memory), erosion,
// binarisation, masks given if M > 0.  Nothing behind m.masks is read.  who: the messages' prefix; cam >= 0: the input of that camera
// of a multi-camera pass
int check_wide_input(lpf_ctx *c, const char *who, int cam, const lpf_wide_input &m, int max_M, const char *takes, const char *more,
                     bool takes_rle = false)
{
    if (m.M < 0 || m.M > max_M) {
        if (cam < 0) return fail(c, LPF_ERR_ARG, "%s: M=%d masks per frame, %s = %d%s", who, m.M, takes, max_M, more);
        return fail(c, LPF_ERR_ARG, "%s: camera %d has M=%d masks per frame, %s = %d%s", who, cam, m.M, takes, max_M, more);
    }
    char w[96];
    if (cam < 0) snprintf(w, sizeof w, "%s", who); else snprintf(w, sizeof w, "%s: camera %d", who, cam);
    if (m.f32 != LPF_MASKS_U8 && m.f32 != LPF_MASKS_F32 && m.f32 != LPF_MASKS_RLE)
        return fail(c, LPF_ERR_ARG, "%s: f32=%d (LPF_MASKS_U8 = 0, LPF_MASKS_F32 = 1 or LPF_MASKS_RLE = 2)", w, m.f32);
    if (m.f32 == LPF_MASKS_RLE && !takes_rle)
        return fail(c, LPF_ERR_ARG, "%s: f32=LPF_MASKS_RLE: lpf_%s takes dense masks only (run-length masks: lpf_run_wide, lpf_run_cams, "
                                    "lpf_run_cams_wide)", w, who);
    if (m.f32 == LPF_MASKS_RLE && m.on_device != 0)
        return fail(c, LPF_ERR_ARG, "%s: f32=LPF_MASKS_RLE with on_device=%d: run-length masks are host memory (on_device 0)", w, m.on_device);
    if (m.erode_iters < 0 || (m.f32 == LPF_MASKS_F32 && (m.binarize < 0 || m.binarize > 2)) || (m.M > 0 && !m.masks))
        return fail(c, LPF_ERR_ARG, "%s: erode_iters=%d f32=%d binarize=%d masks=%p", w, m.erode_iters, m.f32, m.binarize, m.masks);
    return LPF_OK;
}

// The run-length masks of a lpf_wide_input that check_wide_input let through, for a pass of F frames on an image of hw pixels: the
// struct must describe this call (F, M, erode_iters), then lpf_set_masks_rle's walk with the call's prefix (and camera).  R: the checked
// input and its work units (R.in stays NULL for dense masks, and where there is no struct to read).  Nothing is enqueued
int check_wide_rle(lpf_ctx *c, const char *who, int cam, const lpf_wide_input &m, int F, long long hw, lpf_ctx::RleIn &R)
{
    R.in = nullptr; R.Rtot = 0; R.units.clear();
    if (m.f32 != LPF_MASKS_RLE || !m.masks) return LPF_OK;
    char w[96];
    if (cam < 0) snprintf(w, sizeof w, "%s", who); else snprintf(w, sizeof w, "%s: camera %d", who, cam);
    const lpf_rle_masks *in = (const lpf_rle_masks *)m.masks;
    if (in->F != F || in->M != m.M || in->erode_iters != m.erode_iters)
        return fail(c, LPF_ERR_ARG, "%s: the run-length masks say F=%d M=%d erode_iters=%d, the call has F=%d M=%d erode_iters=%d", w, in->F,
                    in->M, in->erode_iters, F, m.M, m.erode_iters);
    int rc;
    if ((rc = rle_walk(c, w, in, hw, R.units, &R.Rtot))) return rc;
    R.in = in;
    return LPF_OK;
}

// the rectangles of a lpf_wide_input hold where lpf_set_mask_rects takes them: uint8, or float under binarize 0, without erosion
bool rects_hold(const lpf_wide_input &m) { return m.rects && m.erode_iters == 0 && (!m.f32 || m.binarize == 0); }

// the masks of a lpf_wide_input (M > 0) for F frames of hw pixels: host masks and rectangles are staged into dm / dr in stream order
// (*host_in is set), device ones are lent.  *rects: the rectangles where they hold (rects_hold), else NULL
int stage_masks(lpf_ctx *c, const lpf_wide_input &m, int F, size_t hw, DevBuf &dm, DevBuf &dr, const void **masks, const int4 **rects,
                bool *host_in)
{
    int rc;
    const void *d_masks = m.masks;
    const int32_t *d_rects = m.rects;
    if (!m.on_device) {
        const size_t bytes = (size_t)F * m.M * hw * (m.f32 ? 4 : 1);
        if ((rc = reserve(c, dm, bytes))) return rc;
        LPF_HIP(c, hipMemcpyAsync(dm.p, m.masks, bytes, hipMemcpyHostToDevice, c->stream));
        d_masks = dm.p;
        if (m.rects) {
            if ((rc = reserve(c, dr, (size_t)F * m.M * 16))) return rc;
            LPF_HIP(c, hipMemcpyAsync(dr.p, m.rects, (size_t)F * m.M * 16, hipMemcpyHostToDevice, c->stream));
            d_rects = (const int32_t *)dr.p;
        }
        *host_in = true;
    }
    *masks = d_masks;
    *rects = rects_hold(m) ? (const int4 *)d_rects : nullptr;
    return LPF_OK;
}

// a camera as the kernels take it (LpfCam): the context's (lpf_set_camera) or a lpf_cam_input's
struct Cam {
    const double *T, *K;              // T: rows 0..2 are used (as lpf_set_camera)
    double dmin, dmax;
    int W, H;
};
Cam ctx_cam(const lpf_ctx *c) { return Cam{c->T, c->K, c->dmin, c->dmax, c->W, c->H}; }
Cam input_cam(const lpf_cam_input &I) { return Cam{I.T_velo_to_rect, I.K, I.depth_min_excl, I.depth_max_excl, I.W, I.H}; }
void set_cam(LpfCam &P, const Cam &k)
{
    memcpy(P.T, k.T, sizeof P.T);
    memcpy(P.K, k.K, sizeof P.K);
    P.dmin = k.dmin; P.dmax = k.dmax; P.W = k.W; P.H = k.H;
}

// The segmentation of a narrow run (lpf_run_batch, lpf_run_cams): segments of 4096 points (1024 for small launches), one list wave
// each; K1 tiles subdivide them; groups of 64 segments are the second level of the counters.  Tail blocks: four consecutive segments
// of one frame each (an empty frame still gets one, to write its summary) -- the list blocks, then, when boxes are counted, a box-count
// block per list block, 64-box word of its frame and part (csplit parts: see lpf_tail_block).
struct NarrowLayout {
    int F = 0;
    bool small = false;
    int64_t seg_pts = 0;
    int nseg_total = 0, ngrp_total = 0, max_ngrp = 0;
    int nblk = 0;                     // list blocks
    int nwblk = 0;                    // list blocks x 64-box words of their frame (at least one): box-count blocks per part
    int csplit = 1, ncblk = 0;        // parts, box-count blocks
    bool few = false;                 // a frame or two (see lpf_run_batch): the lists use the 16-row wave
    bool pre_scan = false;            // segment prefixes from the scan kernel
    int nseg_cap() const { return nseg_total > 0 ? nseg_total : 1; }
    int ngrp_cap() const { return ngrp_total > 0 ? ngrp_total : 1; }
    void split(int parts) { csplit = parts; ncblk = nwblk * parts; }
};

// the frame records of a narrow run (into c->h_frames) and its layout: F frames of frame_off, the boxes of BX, lists of inst_cap entries
void narrow_layout(lpf_ctx *c, const int64_t *frame_off, int F, const lpf_ctx::BoxSet &BX, long long inst_cap, bool small, NarrowLayout &L)
{
    L = NarrowLayout();
    L.F = F; L.small = small;
    L.seg_pts = small ? LPF_SEG_SMALL : LPF_SEG_QUANTUM;
    c->h_frames.resize(F);
    for (int f = 0; f < F; ++f) {
        LpfFrame &fr = c->h_frames[f];
        fr.pt_off = frame_off[f];
        fr.N = (int)(frame_off[f + 1] - frame_off[f]);
        fr.seg_off = L.nseg_total;
        fr.shift = (int)(frame_off[f] & 63);               // the frame's rows start at the 64-point boundary below its first point (LpfFrame)
        fr.nseg = fr.N ? (int)((fr.N + fr.shift + L.seg_pts - 1) / L.seg_pts) : 0;
        L.nseg_total += fr.nseg;
        fr.box_off = BX.F ? BX.box_off[f] : 0;
        fr.B = BX.F ? BX.box_off[f + 1] - BX.box_off[f] : 0;
        fr.inst_base = (long long)f * inst_cap;
        fr.pad = f;
        fr.cand_off = BX.F ? BX.cand_off[f] : 0;
        fr.cand_words = (fr.B + 63) / 64;
        fr.grp_off = L.ngrp_total;
        fr.pad4 = 0;
        const int ngrp = (fr.nseg + LPF_GROUP_SEGS - 1) / LPF_GROUP_SEGS;
        L.ngrp_total += ngrp;
        L.max_ngrp = std::max(L.max_ngrp, ngrp);
        const int nb = fr.nseg > 0 ? (fr.nseg + LPF_LISTS_WAVES - 1) / LPF_LISTS_WAVES : 1;
        L.nblk += nb;
        L.nwblk += nb * std::max(1, fr.cand_words);
    }
    L.few = small && L.nblk <= LPF_FEW_BLOCKS;
    // a list wave sums one group's segments and the frame's groups, a lane each: frames of more than 64 groups (16.7 M points) take
    // their prefixes from the scan kernel instead
    L.pre_scan = L.max_ngrp > 64;
    L.split(1);
}

// ballots and counters of a narrow run of layout L with M masks and Btot boxes in scratch set S
int narrow_reserve(lpf_ctx *c, lpf_ctx::Scratch &S, const NarrowLayout &L, int M, int Btot)
{
    int rc;
    const size_t rows = (size_t)L.nseg_cap() * (size_t)(L.seg_pts / 64);
    if ((rc = reserve(c, S.vbal, rows * 8))) return rc;
    if ((rc = reserve(c, S.mbal, rows * 8))) return rc;
    if ((rc = reserve(c, S.seg_tab, (size_t)LPF_TAB_GROUPS * L.nseg_cap() * sizeof(uint4), true))) return rc;
    if ((rc = reserve(c, S.grp_tab, (size_t)LPF_TAB_GROUPS * L.ngrp_cap() * sizeof(uint4), true))) return rc;
    if ((rc = reserve(c, S.frm_tab, (size_t)L.F * LPF_FRM_SHARDS * LPF_TAB_GROUPS * sizeof(uint4), true))) return rc;
    if (L.pre_scan && (rc = reserve(c, S.seg_pre, (size_t)LPF_TAB_GROUPS * L.nseg_cap() * sizeof(uint4)))) return rc;
    if ((rc = reserve(c, S.cnt, (size_t)(M > 0 ? M : 1) * (Btot > 0 ? Btot : 1) * 4, true))) return rc;
    return LPF_OK;
}

// The geometry tables of a narrow run of layout L in scratch set S: the frame records (c->h_frames), the owning frame's record per
// segment, the list and box-count block tables.  A single frame needs none of them (record by value, block table computed).  They are
// built from the frame records and csplit alone, which the set keeps as their key: only another key uploads them (unless `force`),
// through the pinned ring -- no wait, no drain.
int narrow_tables(lpf_ctx *c, lpf_ctx::Scratch &S, const NarrowLayout &L, bool force)
{
    const int F = L.F;
    if (F <= 1) return LPF_OK;
    const size_t b_frames = (size_t)F * sizeof(LpfFrame), b_segs = (size_t)L.nseg_total * sizeof(LpfFrame), b_blks = (size_t)L.nblk * sizeof(int2),
                 b_cblks = (size_t)L.ncblk * sizeof(int4);
    if (!force && S.tab_csplit == L.csplit && S.tab_frames.size() == (size_t)F && memcmp(S.tab_frames.data(), c->h_frames.data(), b_frames) == 0)
        return LPF_OK;
    int rc;
    if ((rc = reserve(c, S.tab, b_frames + b_segs + b_blks + b_cblks))) return rc;
    c->h_tab.resize(b_frames + b_segs + b_blks + b_cblks);
    memcpy(c->h_tab.data(), c->h_frames.data(), b_frames);
    LpfFrame *hs = reinterpret_cast<LpfFrame *>(c->h_tab.data() + b_frames);
    int2 *hb = reinterpret_cast<int2 *>(c->h_tab.data() + b_frames + b_segs);
    int4 *hc = reinterpret_cast<int4 *>(c->h_tab.data() + b_frames + b_segs + b_blks);
    for (int f = 0; f < F; ++f) {
        const LpfFrame &fr = c->h_frames[f];
        const int wpg = std::max(1, fr.cand_words);
        for (int sg = 0; sg < fr.nseg; ++sg) hs[(size_t)fr.seg_off + sg] = fr;
        if (fr.nseg == 0) {
            *hb++ = make_int2(fr.seg_off, f << 3);
            for (int w = 0; w < wpg; ++w) for (int r = 0; r < L.csplit; ++r) *hc++ = make_int4(fr.seg_off, f, w, r << 3);
        }
        for (int sg = 0; sg < fr.nseg; sg += LPF_LISTS_WAVES) {
            const int nw = std::min(LPF_LISTS_WAVES, fr.nseg - sg);
            *hb++ = make_int2(fr.seg_off + sg, (f << 3) | nw);
            for (int w = 0; w < wpg; ++w) for (int r = 0; r < L.csplit; ++r) *hc++ = make_int4(fr.seg_off + sg, f, w, (r << 3) | nw);
        }
    }
    S.tab_frames.clear();                                  // (nothing valid if the upload fails half way)
    if ((rc = upload(c, S.tab.p, c->h_tab.data(), c->h_tab.size()))) return rc;
    S.tab_frames = c->h_frames;
    S.tab_csplit = L.csplit;
    S.o_segs = b_frames; S.o_blks = b_frames + b_segs; S.o_cblks = b_frames + b_segs + b_blks;
    ++c->generation;                                       // graphs captured for another geometry read these tables
    return LPF_OK;
}

// the parts of a narrow run's parameters that do not depend on its path: camera, shape, tables (narrow_tables), box tables, scratch
// (narrow_reserve).  P is cleared first.
void narrow_params(LpfParams &P, const lpf_ctx *c, const Cam &cam, const NarrowLayout &L, const lpf_ctx::Scratch &S, const lpf_ctx::BoxSet &BX,
                   int M, long long inst_cap)
{
    memset(&P, 0, sizeof P);
    set_cam(P, cam);
    const int Btot = BX.total();
    P.F = L.F; P.M = M; P.seg_pts = (int)L.seg_pts; P.nseg_total = L.nseg_total; P.nseg_cap = L.nseg_cap(); P.ngrp_cap = L.ngrp_cap();
    P.oriented = BX.F ? BX.oriented : 1; P.inst_cap = inst_cap;
    P.frame0 = c->h_frames[0];
    if (L.F > 1) {
        P.frames = (const LpfFrame *)S.tab.p;
        P.segs = (const LpfFrame *)((const char *)S.tab.p + S.o_segs);
        P.blks = (const int2 *)((const char *)S.tab.p + S.o_blks);
        P.cblks = (const int4 *)((const char *)S.tab.p + S.o_cblks);
    }
    P.boxp = (const double *)BX.boxp.p; P.boxq = (const float *)BX.boxq.p;
    P.cand = (const unsigned long long *)BX.cand.p;
    P.vbal = (unsigned long long *)S.vbal.p; P.mbal = (unsigned long long *)S.mbal.p;
    P.seg_tab = (uint4 *)S.seg_tab.p; P.grp_tab = (uint4 *)S.grp_tab.p; P.frm_tab = (uint4 *)S.frm_tab.p;
    P.seg_pre = L.pre_scan ? (uint4 *)S.seg_pre.p : nullptr;
    P.cnt = (unsigned *)S.cnt.p;
    P.nblk = L.nblk; P.ncblk = L.ncblk; P.csplit = L.csplit; P.lists_small = L.few ? 1 : 0; P.count_boxes = (M > 0 && Btot > 0) ? 1 : 0;
    P.count_lazy = L.small ? 0 : 1;
}

// The outputs of a narrow run of n points, F frames, M masks and Btot boxes -> P's pointers: the caller's device pointers, or pieces of
// `buf` for a host caller (narrow_back_a / narrow_back_b copy them back) and for what the run needs though the caller left it out --
// the dense uv / labels the compact copies are gathered from, and the summaries: always produced, host callers size the list copies by
// them.  Every output field of lpf_outputs is bound here and nowhere else.
int narrow_bind(lpf_ctx *c, DevBuf &buf, const lpf_outputs &o, size_t n, int F, int M, int Btot, LpfParams &P)
{
    Stage S(!o.on_device);
    S.add(P.summary, o.summary, sizeof(lpf_frame_summary), (size_t)F, true);
    S.add(P.uv, o.uv, 8, n, o.uv_valid != nullptr);
    S.add(P.label_bits, o.label_bits, 4, n, o.label_valid != nullptr);
    S.add(P.uv_valid, o.uv_valid, 8, n);
    S.add(P.label_valid, o.label_valid, 4, n);
    S.add(P.depth, o.depth, 8, n);
    S.add(P.uf, o.u_f, 8, n);
    S.add(P.vf, o.v_f, 8, n);
    S.add(P.valid_idx, o.valid_idx, 8, n);
    S.add(P.inst_idx, o.inst_idx, 8, (size_t)F * (size_t)(o.inst_cap > 0 ? o.inst_cap : 0));
    S.add(P.count_out, o.count_mb, 4, (size_t)(M > 0 ? M : 1) * (Btot > 0 ? Btot : 1));
    return S.commit(c, buf);
}

// Host outputs of a narrow run of n points, phase (a): the dense arrays are queued.  Then, with result buffers in page-locked memory
// (lpf_host_alloc, hipHostMalloc), lpf_results_to_host writes the filled parts of the compact results and the summaries there, reading
// the lengths from the summaries on the device -- one launch and ONE host wait, where the copy engine needs the summaries on the host
// first (a wait), four copies per frame and a second wait.  Else the counts (nMB = M x Btot) are queued, and the summaries into hs[F]:
// *lists says that the lists are still to be copied (phase b), once the caller has waited for hs.
int narrow_back_a(lpf_ctx *c, const lpf_outputs &o, const LpfParams &P, size_t n, int nMB, lpf_frame_summary *hs, bool *lists)
{
#define LPF_D2H(member, field, bytes) \
    if (o.member && (bytes)) LPF_HIP(c, hipMemcpyAsync(o.member, P.field, (bytes), hipMemcpyDeviceToHost, c->stream));
    LPF_D2H(uv, uv, n * 8)
    LPF_D2H(label_bits, label_bits, n * 4)
    LPF_D2H(depth, depth, n * 8)
    LPF_D2H(u_f, uf, n * 8)
    LPF_D2H(v_f, vf, n * 8)
    LpfToHost D;
    memset(&D, 0, sizeof D);
    bool r2h = o.summary != nullptr && (o.valid_idx || o.inst_idx);
    auto alias = [&](void *host, void **dev) {
        *dev = host ? device_alias_of_pinned(host) : nullptr;
        if (host && !*dev) r2h = false;
    };
    if (r2h) {
        alias(o.summary, &D.summary);
        alias(o.valid_idx, (void **)&D.valid_idx);
        alias(o.uv_valid, (void **)&D.uv_valid);
        alias(o.label_valid, (void **)&D.label_valid);
        alias(o.inst_idx, (void **)&D.inst_idx);
        alias(o.count_mb, (void **)&D.count_mb);
    }
    if (r2h) {
        D.inst_cap = o.inst_cap;
        D.n_count = o.count_mb ? nMB : 0;
        hipLaunchKernelGGL(lpf_results_to_host, dim3((unsigned)P.F * LPF_R2H_BLOCKS), dim3(LPF_BLOCK), 0, c->stream, P, D);
        LPF_HIP(c, hipGetLastError());
        *lists = false;
        return LPF_OK;
    }
    LPF_D2H(count_mb, count_out, (size_t)nMB * 4)
#undef LPF_D2H
    LPF_HIP(c, hipMemcpyAsync(hs, P.summary, (size_t)P.F * sizeof(lpf_frame_summary), hipMemcpyDeviceToHost, c->stream));
    *lists = true;
    return LPF_OK;
}

// phase (b), after the caller's wait: the filled part of each frame's lists, by the summaries hs[F]; the summaries to the caller
int narrow_back_b(lpf_ctx *c, const lpf_outputs &o, const LpfParams &P, const int64_t *frame_off, const lpf_frame_summary *hs)
{
    for (int f = 0; f < P.F; ++f) {
        const size_t nv = (size_t)hs[f].n_valid;
        if (o.valid_idx && nv)
            LPF_HIP(c, hipMemcpyAsync(o.valid_idx + frame_off[f], P.valid_idx + frame_off[f], nv * 8, hipMemcpyDeviceToHost, c->stream));
        if (o.uv_valid && nv)
            LPF_HIP(c, hipMemcpyAsync(o.uv_valid + 2 * frame_off[f], P.uv_valid + frame_off[f], nv * 8, hipMemcpyDeviceToHost, c->stream));
        if (o.label_valid && nv)
            LPF_HIP(c, hipMemcpyAsync(o.label_valid + frame_off[f], P.label_valid + frame_off[f], nv * 4, hipMemcpyDeviceToHost, c->stream));
        int64_t tot = hs[f].inst_off[LPF_MAX_MASKS];
        if (tot > o.inst_cap) tot = o.inst_cap;
        if (o.inst_idx && tot > 0)
            LPF_HIP(c, hipMemcpyAsync(o.inst_idx + (size_t)f * o.inst_cap, P.inst_idx + (size_t)f * o.inst_cap, (size_t)tot * 8,
                                      hipMemcpyDeviceToHost, c->stream));
    }
    if (o.summary) memcpy(o.summary, hs, (size_t)P.F * sizeof(lpf_frame_summary));
    return LPF_OK;
}

// the frame table of a wide run into fr[F]: F frames of frame_off with the boxes of BX.  Returns the chunks; *nbw: the 64-box words of
// the frame with the most boxes
int wide_frames(const int64_t *frame_off, int F, const lpf_ctx::BoxSet &BX, LpfWideFrame *fr, int *nbw)
{
    int nchunk = 0, maxB = 0;
    for (int f = 0; f < F; ++f) {
        LpfWideFrame &e = fr[f];
        e.pt_off = frame_off[f];
        e.N = (int)(frame_off[f + 1] - frame_off[f]);
        e.chunk_off = nchunk;
        e.nchunk = (e.N + LPF_WIDE_CHUNK - 1) / LPF_WIDE_CHUNK;
        e.box_off = BX.F ? BX.box_off[f] : 0;
        e.B = BX.F ? BX.box_off[f + 1] - BX.box_off[f] : 0;
        e.pad = 0;
        nchunk += e.nchunk;
        maxB = std::max(maxB, e.B);
    }
    *nbw = (maxB + 63) / 64;
    return nchunk;
}

// the parts of a wide run's parameters that do not depend on its path: camera, shape, frame table (wide_frames), box tables.  W is
// cleared first; the points, planes, outputs and scratch are the caller's (wide_pack, wide_bind)
void wide_params(LpfWideParams &W, const Cam &cam, int F, int M, int nchunk, int nbw, const lpf_ctx::BoxSet &BX, long long inst_cap,
                 const LpfWideFrame *frames)
{
    memset(&W, 0, sizeof W);
    set_cam(W.cam, cam);
    W.F = F; W.M = M; W.LW = (M + 31) / 32; W.nchunk = nchunk; W.nbw = nbw;
    W.oriented = BX.F ? BX.oriented : 1; W.inst_cap = inst_cap;
    W.frames = frames;
    W.boxp = (const double *)BX.boxp.p; W.boxq = (const float *)BX.boxq.p;
}

}  // namespace

extern "C" {

int lpf_abi_version(void) { return LPF_ABI_VERSION; }

// The sources this binary was compiled from (see include/lpf.h).  The marker string is what _build.library_id() looks for in
// the file, so a stale library is recognised without loading it.
#ifndef LPF_BUILD_ID_STR
#define LPF_BUILD_ID_STR "unknown"
#endif
static const char lpf_build_marker[] = "LPF_BUILD_ID=" LPF_BUILD_ID_STR;
const char *lpf_build_id(void) { return lpf_build_marker + 13; }

void *lpf_host_alloc(size_t bytes)
{
    void *p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) { fail(nullptr, LPF_ERR_NOMEM, "lpf_host_alloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
    return p;
}

void lpf_host_free(void *p) { if (p) (void)hipHostFree(p); }

int lpf_create(lpf_ctx **out, int device_id)
{
    if (!out) return fail(nullptr, LPF_ERR_ARG, "lpf_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, LPF_ERR_HIP, "no HIP device: %s", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(nullptr, LPF_ERR_ARG, "device_id %d out of range [0,%d)", device_id, n);
    lpf_ctx *c = new (std::nothrow) lpf_ctx();
    if (!c) return fail(nullptr, LPF_ERR_NOMEM, "out of host memory");
    c->device = device_id;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
        fail(nullptr, LPF_ERR_HIP, "stream creation failed: %s", hipGetErrorString(e));
        delete c;
        return LPF_ERR_HIP;
    }
    c->own_stream = true;
    *out = c;
    return LPF_OK;
}

void lpf_destroy(lpf_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (auto &S : c->sc) {
        DevBuf *sb[] = {&S.vbal, &S.mbal, &S.seg_tab, &S.grp_tab, &S.frm_tab, &S.seg_pre, &S.cnt, &S.mlist, &S.label_a, &S.label_b, &S.tab, &S.rects, &S.rgrid, &S.out_stage};
        for (DevBuf *b : sb) release(*b);
    }
    for (auto *ring : {c->boxes.ring, c->cams.bx})
        for (int k = 0; k < LPF_NSETS; ++k) {
            lpf_ctx::BoxSet &B = ring[k];
            DevBuf *bb[] = {&B.boxp, &B.boxq, &B.cand, &B.corners, &B.enabled, &B.aux, &B.bframes, &B.stage};
            for (DevBuf *b : bb) release(*b);
        }
    for (int k = 0; k < LPF_NSETS; ++k) {
        DevBuf *cb[] = {&c->cams.label_a[k], &c->cams.label_b[k], &c->cams.masks[k], &c->cams.rects[k], &c->cams.rle[k], &c->cams.out[k]};
        for (DevBuf *b : cb) release(*b);
    }
    release(c->cams.pts);
    for (lpf_ctx::Wide *D : {&c->wide, &c->camsw.cam[0], &c->camsw.cam[1], &c->camsw.cam[2], &c->camsw.cam[3]}) {
        DevBuf *wb[] = {&D->tab, &D->masks, &D->rects, &D->rle, &D->ids, &D->planes_a, &D->planes_b, &D->flags, &D->ccnt, &D->cpre, &D->fcnt, &D->midx, &D->mwords,
                        &D->mpts, &D->cnt, &D->pts, &D->out};
        for (DevBuf *b : wb) release(*b);
    }
    release(c->camsw.tab);
    release(c->camsw.pts);
    for (DevBuf *b : {&c->dmaps.pack.planes_a, &c->dmaps.pack.planes_b, &c->dmaps.pack.rle, &c->fmat.pack.planes_a, &c->fmat.pack.planes_b,
                      &c->fmat.pack.rle, &c->dmaps.foff, &c->dmaps.win, &c->dmaps.cnt, &c->dmaps.in,
                      &c->dmaps.pts, &c->dmaps.out})
        release(*b);
    for (lpf_ctx::CallBufs *D : {&c->dovl, &c->m2d, &c->insd, &c->bpts, &c->bviews, &c->asgn, (lpf_ctx::CallBufs *)&c->fmat})
        for (DevBuf *b : {&D->tab, &D->pts, &D->in, &D->out}) release(*b);
    release(c->fmat.code);
    release(c->fmat.tiles);
    DevBuf *all[] = {&c->resize_buf, &c->lab_clk, &c->mask_stage, &c->rle_stage, &c->ids_stage, &c->pib_box, &c->pib_pts, &c->pib_out, &c->boxprep, &c->dimg, &c->coll, &c->st_pts, &c->out_stage};
    for (DevBuf *b : all) release(*b);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ring.ev) if (e) (void)hipEventDestroy(e);
    if (c->ring.base) (void)hipHostFree(c->ring.base);
    if (c->pin_back.p) (void)hipHostFree(c->pin_back.p);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char *lpf_last_error(const lpf_ctx *c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int lpf_set_stream(lpf_ctx *c, void *s)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    { int rc_ = sync_all(c); if (rc_) return rc_; }
    if (c->own_stream) { (void)hipStreamDestroy(c->stream); c->own_stream = false; }
    c->stream = (hipStream_t)s;          // NULL is the null stream itself (torch's default stream has handle 0)
    ++c->generation;
    return LPF_OK;
}

int lpf_use_own_stream(lpf_ctx *c)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    { int rc_ = sync_all(c); if (rc_) return rc_; }
    if (c->own_stream) return LPF_OK;
    c->stream = nullptr;
    LPF_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
    ++c->generation;
    return LPF_OK;
}

// ---- explicit ordering against the caller's other streams (no device-wide synchronisation) ---------------
int lpf_wait_for_stream(lpf_ctx *c, void *producer)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (c->capturing) return fail(c, LPF_ERR_STATE, "lpf_wait_for_stream inside graph capture");
    if ((hipStream_t)producer == c->stream) return LPF_OK;      // same stream: already ordered
    hipEvent_t e;
    LPF_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipError_t r = hipEventRecord(e, (hipStream_t)producer);
    if (r == hipSuccess) r = hipStreamWaitEvent(c->stream, e, 0);
    (void)hipEventDestroy(e);                                  // released once it has completed
    if (r != hipSuccess) return fail(c, LPF_ERR_HIP, "lpf_wait_for_stream: %s", hipGetErrorString(r));
    return LPF_OK;
}

int lpf_release_to_stream(lpf_ctx *c, void *consumer)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (c->capturing) return fail(c, LPF_ERR_STATE, "lpf_release_to_stream inside graph capture");
    { int rc_ = flush_pending(c); if (rc_) return rc_; }
    if (c->stream == (hipStream_t)consumer) return LPF_OK;
    hipEvent_t e;
    LPF_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipError_t r = hipEventRecord(e, c->stream);
    if (r == hipSuccess) r = hipStreamWaitEvent((hipStream_t)consumer, e, 0);
    (void)hipEventDestroy(e);
    if (r != hipSuccess) return fail(c, LPF_ERR_HIP, "lpf_release_to_stream: %s", hipGetErrorString(r));
    return LPF_OK;
}

int lpf_sync(lpf_ctx *c)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    return sync_all(c);
}

#ifdef LPF_LAB
// Lab builds only (liblpf_lab.so: tools/ and the forced-geometry fuzz tests): override the launch geometry a run would pick
// by its size.  0 = by launch size, 1 = small with the wide tail, 2 = large, 3 = large with the segment prefixes taken from
// the scan kernel, 4 = small with the narrow tail.  Results do not depend on it.
int lpf_set_geometry(lpf_ctx *c, int mode)
{
    if (!c) return LPF_ERR_ARG;
    if (mode < 0 || mode > 5) return fail(c, LPF_ERR_ARG, "lpf_set_geometry: mode=%d (0 by launch size, 1 small with the wide tail, 2 large, 3 large with scan-kernel prefixes, 4 small with the narrow tail, 5 small with 1024-point tiles)", mode);
    c->geometry = mode;
    ++c->generation;
    return LPF_OK;
}

// Role clock of the step launches (software-pipelined modes): out[6][5] = per role {first block start, last block end, sum of the
// block durations, blocks, longest block} in ticks of the 100 MHz wall clock, accumulated since the last reset.  The first call
// switches the clock on (the step kernel of a lab build then ends every block with a barrier and four atomics).  Synchronises.
int lpf_lab_role_clock(lpf_ctx *c, unsigned long long *out, int reset)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    int rc = sync_all(c);
    if (rc) return rc;
    unsigned long long init[30];
    for (int r = 0; r < 6; ++r) { init[5 * r] = ~0ull; init[5 * r + 1] = init[5 * r + 2] = init[5 * r + 3] = init[5 * r + 4] = 0ull; }
    if (!c->lab_clk.p) {
        if ((rc = reserve(c, c->lab_clk, sizeof init))) return rc;
        if (hipMemcpy(c->lab_clk.p, init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) return fail(c, LPF_ERR_HIP, "lpf_lab_role_clock: hipMemcpy");
    }
    if (out && hipMemcpy(out, c->lab_clk.p, sizeof init, hipMemcpyDeviceToHost) != hipSuccess) return fail(c, LPF_ERR_HIP, "lpf_lab_role_clock: hipMemcpy");
    if (reset && hipMemcpy(c->lab_clk.p, init, sizeof init, hipMemcpyHostToDevice) != hipSuccess) return fail(c, LPF_ERR_HIP, "lpf_lab_role_clock: hipMemcpy");
    return LPF_OK;
}

// Range limits of the batched analysis calls, so that small batches reach the second and later ranges of large ones (plan_ranges, and
// the frame loops of lpf_inside_masks and lpf_box_points): 0 = the product's value; max_items never raises a product limit.
int lpf_lab_set_range_limits(lpf_ctx *c, long long stage_budget_bytes, int max_items)
{
    if (!c) return LPF_ERR_ARG;
    if (stage_budget_bytes < 0 || max_items < 0)
        return fail(c, LPF_ERR_ARG, "lpf_lab_set_range_limits: stage_budget_bytes=%lld max_items=%d (neither may be negative; 0 = the product's value)", stage_budget_bytes, max_items);
    c->lab_budget = stage_budget_bytes;
    c->lab_max_items = max_items;
    return LPF_OK;
}

int lpf_lab_last_ranges(lpf_ctx *c) { return c ? c->lab_ranges : LPF_ERR_ARG; }
#endif

// Rectangles for the masks of the NEXT lpf_set_masks_* call: rects[F][M] = {x0, y0, x1, y1}, half open, pixels; the caller's
// word that mask m of frame f is zero outside its rectangle (a detector's masks are cropped to their boxes).  A hint: where uint8
// masks are packed as they are (no erosion) the pack skips the 16-pixel groups that lie outside; every other form reads the masks in
// full.  Results are those without the hint as long as the caller's word holds.  on_device: 0 host memory (copied now, no wait),
// else device memory read when the masks are packed (it must stay unchanged until then, like lent masks).  NULL clears.
int lpf_set_mask_rects(lpf_ctx *c, const int32_t *rects, int on_device, int F, int M)
{
    if (!c) return LPF_ERR_ARG;
    c->rects_pending = nullptr; c->rects_F = 0; c->rects_M = 0;
    if (!rects || F <= 0 || M <= 0) return LPF_OK;
    if (M > LPF_MAX_MASKS) return fail(c, LPF_ERR_ARG, "lpf_set_mask_rects: M=%d (at most %d)", M, LPF_MAX_MASKS);
    if (use_device(c)) return LPF_ERR_HIP;
    const size_t bytes = (size_t)F * M * sizeof(int4);
    if (on_device) {
        if (((uintptr_t)rects & 15) != 0) return fail(c, LPF_ERR_ARG, "lpf_set_mask_rects: the device array must be 16-byte aligned");
        c->rects_pending = (const int4 *)rects;
    } else {
        if (c->capturing) return LPF_OK;                    // (a copy from host memory is not captured: the hint is dropped)
        // the copy lives in the scratch set of the run these masks are for: in the pipelined modes that run's tiles may read the
        // rectangles a launch after the NEXT run's have been uploaded (into the next set); stream-ordered behind the set's last run
        DevBuf &rb = c->sc[c->pipe.set_now()].rects;
        int rc = reserve(c, rb, bytes);
        if (rc) return rc;
        if ((rc = upload(c, rb.p, rects, bytes))) return rc;
        c->rects_pending = (const int4 *)rb.p;
    }
    c->rects_F = F; c->rects_M = M;
    return LPF_OK;
}

// The erosion element of every erosion the context performs from now on: cv2.getStructuringElement(MORPH_ELLIPSE, (ksize, ksize)), see
// include/lpf.h.  Row |dy| of the element with radius r holds the columns -dx .. dx, dx = LPF_ELLIPSE_DX[r][|dy|]:
// round(r * sqrt((r*r - dy*dy) / (r*r))), shipped as a table (no quotient lies near a tie, so it does not depend on the rounding rule).
// Host state only: nothing is enqueued; masks already packed and a captured graph keep the element they were made with (it is a kernel
// argument).
static const uint8_t LPF_ELLIPSE_DX[8][8] = {{0}, {1, 0}, {2, 2, 0}, {3, 3, 2, 0}, {4, 4, 3, 3, 0}, {5, 5, 5, 4, 3, 0}, {6, 6, 6, 5, 4, 3, 0},
                                             {7, 7, 7, 6, 6, 5, 4, 0}};
int lpf_set_erosion_element(lpf_ctx *c, int ksize)
{
    if (!c) return LPF_ERR_ARG;
    if (ksize < 1 || ksize > 15 || ksize % 2 == 0)
        return fail(c, LPF_ERR_ARG, "lpf_set_erosion_element: ksize=%d (the k x k MORPH_ELLIPSE for odd k, 1 .. 15)", ksize);
    const int r = ksize / 2;
    uint32_t spans = 0;
    for (int j = 0; j <= r; ++j) spans |= (uint32_t)LPF_ELLIPSE_DX[r][j] << (4 * j);
    c->erode_k = ksize; c->erode_r = r; c->erode_spans = spans;
    return LPF_OK;
}

int lpf_set_pipelined(lpf_ctx *c, int on)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (on == 1 || on == 3)
        return fail(c, LPF_ERR_ARG, "lpf_set_pipelined: modes 1 and 3 (tail kernels / mask pack on side streams) were removed in ABI 5 -- "
                                    "they measured slower than 2 and 4 on every workload (DESIGN.md section 8); use 2 or 4");
    if (on != 0 && on != 2 && on != 4) return fail(c, LPF_ERR_ARG, "lpf_set_pipelined: mode %d (0 off, 2 the tail rides in the next run's launch, "
                                                                   "4 = 2 + the mask pack rides as well)", on);
    int rc = sync_all(c);
    if (rc) return rc;
    if ((rc = pack_unpacked(c))) return rc;                // masks that were waiting for a run: packed now, where the next run looks
    c->pipe.fused = on != 0;
    c->pipe.defer = on == 4;
    c->pipe.parity = 0;
    if (c->masks.F && c->masks.set != 0) c->masks.drop();  // label images rotate with the sets: set the masks again
    ++c->generation;
    return LPF_OK;
}

int lpf_set_camera(lpf_ctx *c, const double T[16], const double K[9], int W, int H, double dmin, double dmax)
{
    if (!c) return LPF_ERR_ARG;
    if (!T || !K || W <= 0 || H <= 0 || (long long)W * H > (1ll << 30))
        return fail(c, LPF_ERR_ARG, "set_camera: T=%p K=%p W=%d H=%d", (const void *)T, (const void *)K, W, H);
    // pipelined modes: a run still owed projects / counts boxes with the OLD camera (its box job).  Tables already built stay as they
    // are: they hold velodyne-frame geometry and the visibility decided when they were built, nothing of K, W, H (box state)
    if (!c->capturing && (c->pipe.owes() || c->boxes.in_force().job_valid)) {
        if (use_device(c)) return LPF_ERR_HIP;
        int rc_ = sync_all(c);
        if (rc_) return rc_;
    }
    if (W != c->W || H != c->H) {            // label images (and the visibility filter of cam-0 boxes) are per W x H: set masks / boxes again
        c->masks.drop();
        c->boxes.drop();
    }
    memcpy(c->T, T, sizeof c->T);          // row 3 of the 4x4 is never used by the reference either (V3:567 [:, :3])
    memcpy(c->K, K, sizeof c->K);
    c->W = W; c->H = H; c->dmin = dmin; c->dmax = dmax;
    c->have_camera = true;
    ++c->generation;                         // T, K, W, H are kernel arguments of a captured graph
    return LPF_OK;
}

int lpf_set_masks_u8(lpf_ctx *c, const uint8_t *masks, int F, int M, int erode_iters, int on_device)
{
    return set_masks_impl<uint8_t>(c, masks, F, M, 0, erode_iters, on_device);
}

int lpf_set_masks_f32(lpf_ctx *c, const float *masks, int F, int M, int binarize, int erode_iters, int on_device)
{
    if (c && (binarize < 0 || binarize > 2)) return fail(c, LPF_ERR_ARG, "lpf_set_masks_f32: binarize=%d (0, 1 or 2)", binarize);
    return set_masks_impl<float>(c, masks, F, M, binarize + 1, erode_iters, on_device);
}

// Run-length masks (include/lpf.h): checked in full on the host, which also emits the work units of the decode (lpf_rle.hip.h); then
// set_masks_compact with zero + decode (+ erosion on the packed image).
int lpf_set_masks_rle(lpf_ctx *c, const lpf_rle_masks *in)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (!c->have_camera) return fail(c, LPF_ERR_STATE, "lpf_set_camera must be called before masks (W, H)");
    if (c->capturing)
        return fail(c, LPF_ERR_STATE, "lpf_set_masks_rle cannot be captured into a graph (the run counts size its launch: call it outside "
                                      "lpf_graph_begin ... lpf_graph_end)");
    if (!in) return fail(c, LPF_ERR_ARG, "lpf_set_masks_rle: in=NULL");
    if (in->M > LPF_MAX_MASKS) return too_many_masks(c, in->M);
    RleCall R(c);
    int rc;
    if ((rc = R.walk("lpf_set_masks_rle", in, c->W, c->H))) return rc;
    return set_masks_compact(c, in->F, in->M, [&](lpf_ctx::Scratch &S, int lb, void **cur, bool *host_in) {
        return rle_label_image(c, S.label_a, S.label_b, c->rle_stage, R.A, c->W, c->H, lb, cur, host_in);
    });
}

// Instance-ID maps (include/lpf.h): the struct is checked before anything is queued, then set_masks_compact with ONE decode launch that
// writes every element (+ erosion on the packed image); only a host map is waited for (sel was copied at the call).
int lpf_set_masks_ids(lpf_ctx *c, const lpf_id_masks *in)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (!c->have_camera) return fail(c, LPF_ERR_STATE, "lpf_set_camera must be called before masks (W, H)");
    if (c->capturing)
        return fail(c, LPF_ERR_STATE, "lpf_set_masks_ids cannot be captured into a graph (the table of selected IDs is a host copy: call it "
                                      "outside lpf_graph_begin ... lpf_graph_end)");
    if (!in) return fail(c, LPF_ERR_ARG, "lpf_set_masks_ids: in=NULL");
    if (in->M > LPF_MAX_MASKS) return too_many_masks(c, in->M);
    int rc;
    if ((rc = check_ids(c, "lpf_set_masks_ids", in, (size_t)c->W * c->H))) return rc;
    return set_masks_compact(c, in->F, in->M, [&](lpf_ctx::Scratch &S, int lb, void **cur, bool *host_in) {
        return ids_label_image(c, S.label_a, S.label_b, c->ids_stage, in, c->W, c->H, lb, cur, host_in);
    });
}

int lpf_set_label_image(lpf_ctx *c, const uint32_t *label, int F, int M, int on_device)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (!c->have_camera) return fail(c, LPF_ERR_STATE, "lpf_set_camera must be called first");
    if (F < 0 || M < 0 || M > LPF_MAX_MASKS || (F > 0 && !label)) return fail(c, LPF_ERR_ARG, "set_label_image: F=%d M=%d", F, M);
    int rc;
    if ((rc = sync_all(c))) return rc;
    lpf_ctx::Scratch &S = c->sc[c->pipe.set_now()];
    // (masks a pipelined lpf_set_masks_* left unpacked stay on record, and the next fused run takes them, not this image.  Kept as it was)
    c->masks.begin(c->pipe.set_now());
    if (F == 0) return LPF_OK;
    const size_t bytes = (size_t)F * c->H * c->W * 4;
    if ((rc = reserve(c, S.label_a, bytes))) return rc;
    LPF_HIP(c, hipMemcpyAsync(S.label_a.p, label, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    LPF_HIP(c, host_wait(c));
    c->masks.packed(F, M, S.label_a.p, 4);
    return LPF_OK;
}

int lpf_get_label_image(lpf_ctx *c, uint32_t *out, int on_device)
{
    if (!c || !out) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    { int rc_ = sync_all(c); if (rc_) return rc_; }
    { int rc_ = pack_unpacked(c); if (rc_) return rc_; }
    const lpf_ctx::Masks &MK = c->masks;
    if (!MK.img || !MK.F) return fail(c, LPF_ERR_STATE, "no masks set");
    const size_t npix = (size_t)MK.F * c->H * c->W;
    if (MK.bytes == 4) {
        LPF_HIP(c, hipMemcpyAsync(out, MK.img, npix * 4, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
        LPF_HIP(c, host_wait(c));
        return LPF_OK;
    }
    // narrow label images (M <= 16) are widened on the host: this entry point exists for tests
    std::vector<uint8_t> raw(npix * (size_t)MK.bytes);
    LPF_HIP(c, hipMemcpyAsync(raw.data(), MK.img, raw.size(), hipMemcpyDeviceToHost, c->stream));
    LPF_HIP(c, host_wait(c));
    std::vector<uint32_t> wide(npix);
    for (size_t i = 0; i < npix; ++i)
        wide[i] = MK.bytes == 1 ? (uint32_t)raw[i] : (uint32_t)reinterpret_cast<const uint16_t *>(raw.data())[i];
    LPF_HIP(c, hipMemcpyAsync(out, wide.data(), npix * 4, on_device ? hipMemcpyHostToDevice : hipMemcpyHostToHost, c->stream));
    LPF_HIP(c, host_wait(c));
    return LPF_OK;
}

int lpf_set_boxes(lpf_ctx *c, const double *corners, const int32_t *box_off, int F, int oriented)
{
    return lpf_set_boxes_ex(c, corners, 0, box_off, F, oriented);
}

int lpf_set_boxes_ex(lpf_ctx *c, const double *corners, int on_device, const int32_t *box_off, int F, int oriented)
{
    return set_boxes_impl(c, corners, on_device, box_off, F, oriented, false, nullptr, 0, nullptr, nullptr, nullptr, nullptr, "set_boxes");
}

int lpf_set_boxes_cam0(lpf_ctx *c, const double *corners_cam0, int on_device, const int32_t *box_off, int F, const double Tcv[16],
                       int filter_visible, int oriented, uint8_t *visible, double *corners_velo, double *bbox2d, int32_t *front)
{
    return set_boxes_impl(c, corners_cam0, on_device, box_off, F, oriented, true, Tcv, filter_visible, visible, corners_velo, bbox2d, front,
                          "set_boxes_cam0");
}

int lpf_run_batch(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_outputs *out)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (!c->have_camera) return fail(c, LPF_ERR_STATE, "lpf_set_camera has not been called");
    if (!out || !frame_off || F <= 0) return fail(c, LPF_ERR_ARG, "run: out=%p frame_off=%p F=%d", (const void *)out, (const void *)frame_off, F);
    int rc;
    if ((rc = check_frames(c, "run", pts, frame_off, F, LPF_SEG_QUANTUM))) return rc;
    const int64_t Ntot = frame_off[F];
    lpf_ctx::BoxSet &BX = c->boxes.in_force();
    if (c->masks.F != 0 && c->masks.F != F) return fail(c, LPF_ERR_STATE, "masks were set for %d frames, run has %d", c->masks.F, F);
    if (BX.F != 0 && BX.F != F) return fail(c, LPF_ERR_STATE, "boxes were set for %d frames, run has %d", BX.F, F);
    if (out->inst_idx && out->inst_cap <= 0) return fail(c, LPF_ERR_ARG, "run: inst_idx given with inst_cap=%lld", (long long)out->inst_cap);
    if ((out->uv_valid || out->label_valid) && !out->valid_idx)
        return fail(c, LPF_ERR_ARG, "run: uv_valid / label_valid need valid_idx as well (they share its order)");
    const int M = c->masks.F ? c->masks.M : 0;
    const int Btot = BX.total();
    const bool host_io = !out->on_device;

    // ---- segmentation (NarrowLayout) ---------------------------------------------------------------------------------------------
    const bool small = c->geometry == 1 || c->geometry == 4 || c->geometry == 5 || (c->geometry == 0 && Ntot <= LPF_SMALL_LAUNCH);
    NarrowLayout L;
    narrow_layout(c, frame_off, F, BX, out->inst_cap, small, L);
    // software-pipelined device runs rotate through the scratch sets (3 in mode 2, 4 in mode 4); everything else uses set 0 with
    // nothing owed
    const bool fused = c->pipe.fused && !host_io && pts_on_device;   // one launch per run, the tail rides in the next
    // a frame or two of a real scan (up to 64 list blocks = 262 144 points): the launch is as long as its longest block, so the count
    // blocks are cut in four and the lists use the 16-row wave.  Beyond that both cost more than they save (same box, us per step in a
    // pipelined stream with / without: 20 real frames 29.8 / 25.5 with the cut, 25.2 / 25.5 with the list wave; one 2 M-point
    // synthetic cloud 25.7 / 21.3 and 22.9 / 21.3, in order 42.4 / 38.9 with the list wave).
    L.split(fused && L.few ? 4 : 1);
    if (c->geometry == 3) L.pre_scan = true;
    if (!fused && c->pipe.owes() && (rc = sync_all(c))) return rc;
    lpf_ctx::Scratch &S = c->sc[c->pipe.run_set(fused)];
    if ((rc = narrow_reserve(c, S, L, M, Btot))) return rc;
    if ((rc = narrow_tables(c, S, L, false))) return rc;
    LpfParams P;
    narrow_params(P, c, ctx_cam(c), L, S, BX, M, out->inst_cap);
    const bool sparse_frames = Ntot * 2 <= (int64_t)F * c->W * c->H;
    TileSource src;
    if ((rc = plan_tile_source(c, fused, small, sparse_frames, M, src))) return rc;
    P.label_img = src.img;
    P.rects = src.rects;
    // tiles that read the masks inside their rectangles look a point's candidates up in a coarse grid of the rectangles (a few KB per
    // frame), built once per run: by blocks of this run's own launch where the tiles come a launch later (mode 4), else by a small
    // kernel ahead of the tiles
    LpfRectJob RG;
    memset(&RG, 0, sizeof RG);
    const bool rect_tiles = src.kind == TileSource::DIRECT_RECT;
    if (rect_tiles) {
        RG.rects = P.rects; RG.F = F; RG.M = M;
        RG.cw = (c->W + LPF_RG_CELL - 1) / LPF_RG_CELL; RG.ch = (c->H + LPF_RG_CELL - 1) / LPF_RG_CELL;
        RG.cells = RG.cw * RG.ch; RG.bpf = (RG.cells + LPF_BLOCK - 1) / LPF_BLOCK;
        if ((rc = reserve(c, S.rgrid, (size_t)F * RG.cells * sizeof(uint32_t)))) return rc;
        RG.grid = (uint32_t *)S.rgrid.p;
        P.rect_grid = RG.grid; P.rg_cw = RG.cw; P.rg_cells = RG.cells;
    }

    // ---- buffers: caller's HBM pointers, or internal staging for host callers -----------
    const size_t n = (size_t)Ntot;
    if (pts_on_device) {
        P.pts = (const float4 *)pts;
    } else {
        if ((rc = reserve(c, c->st_pts, n * 16))) return rc;
        if (n) LPF_HIP(c, hipMemcpyAsync(c->st_pts.p, pts, n * 16, hipMemcpyHostToDevice, c->stream));
        P.pts = (const float4 *)c->st_pts.p;
    }
    // (a pipelined run's own pieces -- the dense labels or pixels its compact copies are gathered from, the summaries -- live in its
    //  scratch set: in the context's one buffer the next run's tiles overwrote the labels this run's tail had yet to read)
    if ((rc = narrow_bind(c, fused ? S.out_stage : c->out_stage, *out, n, F, M, Btot, P))) return rc;
    if (M > 0) {                         // K1 -> tail hand-off of the masked points (sparse writes into N slots)
        if ((rc = reserve(c, S.mlist, n * 16))) return rc;
        P.mlist = (float4 *)S.mlist.p;
    }

    c->boxes.claimed_by_run();           // this run's tail counts into the box tables in force

    // small clouds: 512-point tiles (more, shorter blocks); large batches: 1024-point tiles
    // Small geometry: 512-point tiles while they fit the chip's block slots in one round (256 CUs x 7 blocks: a real frame is 214
    // tiles, a launch of a few frames a few hundred), one 1024-point tile per segment beyond -- a single mid-size cloud in 512-point
    // tiles pays for a third, nearly empty round of blocks (one cloud per launch set, in order / pipelined, us: 1 M points 43.6 / 17.4
    // -> 38.7 / 14.7, 2 M 39.2 / 21.4 -> 37.6 / 20.5, 3 M 63.9 / 28.4 -> 45.5 / 26.8).  Not for tiles that read M mask values per
    // valid point (LpfDirect: 512-point form only; small sparse launches).  Lab geometry 5 forces the 1024-point form, 1 / 4 the other.
    const bool small_1024 = small && src.kind != TileSource::DIRECT && (c->geometry == 5 || (c->geometry == 0 && Ntot > 1792ll * 512));
    P.tile_pts = small ? (small_1024 ? 1024 : 512) : 1024;
    // the fused launch shares the chip with the previous run's tail blocks: 2048-point tiles keep twice the loads in flight
    // per wave, so the streaming work holds its bandwidth on fewer resident blocks (measured: 104.9 vs 108.8 us per step)
    if (fused && !small) P.tile_pts = rect_tiles ? LPF_RECT_FUSED_TILE : 2048;
    const int nk1 = L.nseg_total * (int)(L.seg_pts / P.tile_pts);
    const bool want_lists = out->valid_idx || out->inst_idx;
    const int ntail = (P.count_boxes ? L.ncblk : 0) + (want_lists ? L.nblk : 0);        // no lists wanted and no boxes: no tail blocks at all
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // mode 4: the mask pack and the tiles of one launch share the label element type -- else the pipeline is drained first
    if (fused && c->pipe.must_drain_before(src) && (rc = flush_pending(c))) return rc;
    // the candidate grid of the masks' rectangles: where this run's tiles are in this run's own launch(es) -- in order, mode 2 -- a
    // small kernel ahead of them; in mode 4 it rides in the launch below (the tiles come a launch later)
    const bool tiles_wait = fused && c->pipe.defer;        // this run's tiles go into the NEXT launch
    if (rect_tiles && nk1 > 0 && !tiles_wait) {
        hipLaunchKernelGGL(lpf_rect_grid_kernel, dim3((unsigned)(RG.F * RG.bpf)), dim3(LPF_BLOCK), 0, c->stream, RG);
        LPF_HIP(c, hipGetLastError());
    }
    // (profiling brackets the launches that carry streaming tiles: in mode 4 the first launch after a drain carries none)
    const bool carries_k1 = fused ? c->pipe.next_carries_tiles() : nk1 > 0;
    if (carries_k1 && c->profiling && c->ev_used < (1u << 16)) {
        if (c->ev.size() < 2 * (c->ev_used + 1)) {
            hipEvent_t a, b;
            LPF_HIP(c, hipEventCreate(&a));
            LPF_HIP(c, hipEventCreate(&b));
            c->ev.push_back(a); c->ev.push_back(b);
        }
        e0 = c->ev[2 * c->ev_used]; e1 = c->ev[2 * c->ev_used + 1];
        ++c->ev_used;
        LPF_HIP(c, hipEventRecord(e0, c->stream));
    }
    if (fused) {
        // ---- one launch (lpf_step_t): K1 tiles, the tail blocks of the run before dealt out among them, the summaries of the
        //      run before that, and the box job of THIS run (its tables are read by this run's tail, one or two launches on).
        //      Mode 2: the tiles are this run's.  Mode 4: this run's MASK PACK rides as well (lent uint8 masks), the tiles are
        //      the previous run's -- everything one launch later, nothing left on the stream between two steps.
        const lpf_ctx::Pending cur = pending_run(P, L.pre_scan, ntail, nk1, src);
        if ((rc = queue_step(c, &cur, &BX, e1, (rect_tiles && tiles_wait) ? &RG : nullptr))) return rc;
        c->masks.forget_unpacked();
        c->pipe.parity = (c->pipe.parity + 1) % c->pipe.sets();
        return LPF_OK;
    }
    if (BX.job_ready() && nk1 > 0) {
        // in order, with a box job waiting: the tiles and the job share one launch (lpf_step_t with those two roles), the tail
        // that reads the tables follows in the next -- the same number of launches as with boxes that never change
        const lpf_ctx::Pending cur = pending_run(P, false, 0, nk1, src);
        lpf_ctx::Pending none;
        if ((rc = launch_step(c, cur, none, none, nullptr, &BX, e1))) return rc;
    } else {
    if ((rc = launch_box_job(c, BX))) return rc;           // (no tiles to ride with)
    if (nk1 > 0) {
        const dim3 g1((unsigned)nk1);
        with_tile_form<false>(src, P.tile_pts >> 8, false, [&](auto lt, auto rw, auto) {
            hipLaunchKernelGGL((lpf_k1_project_t<decltype(rw)::value, LPF_K1_FLAGS, typename decltype(lt)::type>), g1, dim3(LPF_BLOCK), 0, c->stream, P);
        });
        LPF_HIP(c, hipGetLastError());
        if (e1) LPF_HIP(c, hipEventRecord(e1, c->stream));
    }
    }
    // ---- the tail: lists and box counts in one launch (a wave per segment each, side by side), then the per-frame summaries ----
    if (L.pre_scan && L.nseg_total > 0) {
        hipLaunchKernelGGL(lpf_scan_segments, dim3(F), dim3(LPF_BLOCK), 0, c->stream, P);
        LPF_HIP(c, hipGetLastError());
    }
    if (ntail > 0) {
        if (small && P.count_boxes && c->geometry != 4 && (L.nblk <= LPF_WIDE_BELOW || c->geometry == 1)) {   // a frame or a few, dense real segments: the box-count blocks share their chunks over 16 waves
            if (L.pre_scan) hipLaunchKernelGGL((lpf_tail_wide_t<true>), dim3((unsigned)ntail), dim3(64 * LPF_WIDE_WAVES), 0, c->stream, P);
            else hipLaunchKernelGGL((lpf_tail_wide_t<false>), dim3((unsigned)ntail), dim3(64 * LPF_WIDE_WAVES), 0, c->stream, P);
        } else {
            launch_tail(c->stream, P, ntail, L.pre_scan);
        }
        LPF_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(lpf_finalize, dim3(F), dim3(LPF_BLOCK), 0, c->stream, P);
    LPF_HIP(c, hipGetLastError());

    if (host_io) {
        std::vector<lpf_frame_summary> hs((size_t)F);
        bool lists = false;
        if ((rc = narrow_back_a(c, *out, P, n, M * Btot, hs.data(), &lists))) return rc;
        LPF_HIP(c, host_wait(c));
        if (lists) {
            if ((rc = narrow_back_b(c, *out, P, frame_off, hs.data()))) return rc;
            LPF_HIP(c, host_wait(c));
        }
    }
    return LPF_OK;
}

int lpf_points_in_boxes(lpf_ctx *c, const float *pts, int64_t k, int stride, const double *corners, int B, int oriented,
                        uint8_t *inside, int on_device)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (k < 0 || B < 0 || (stride != 3 && stride != 4) || (k > 0 && !pts) || (B > 0 && !corners) || (k > 0 && B > 0 && !inside))
        return fail(c, LPF_ERR_ARG, "points_in_boxes: k=%lld B=%d stride=%d", (long long)k, B, stride);
    if (k == 0 || B == 0) return LPF_OK;
    std::vector<double> bp((size_t)B * 16);
    for (int b = 0; b < B; ++b) box_params(corners + (size_t)b * 24, oriented, bp.data() + (size_t)b * 16);
    int rc;
    if ((rc = reserve(c, c->pib_box, bp.size() * 8))) return rc;
    LPF_HIP(c, hipMemcpyAsync(c->pib_box.p, bp.data(), bp.size() * 8, hipMemcpyHostToDevice, c->stream));
    const float *d_pts = pts;
    uint8_t *d_out = inside;
    if (!on_device) {
        if ((rc = reserve(c, c->pib_pts, (size_t)k * stride * 4))) return rc;
        if ((rc = reserve(c, c->pib_out, (size_t)k * B))) return rc;
        LPF_HIP(c, hipMemcpyAsync(c->pib_pts.p, pts, (size_t)k * stride * 4, hipMemcpyHostToDevice, c->stream));
        d_pts = (const float *)c->pib_pts.p; d_out = (uint8_t *)c->pib_out.p;
    }
    hipLaunchKernelGGL(lpf_points_in_boxes_kernel, dim3((unsigned)((k + LPF_BLOCK - 1) / LPF_BLOCK)), dim3(LPF_BLOCK), 0, c->stream,
                       d_pts, (long long)k, stride, (const double *)c->pib_box.p, B, oriented ? 1 : 0, d_out);
    LPF_HIP(c, hipGetLastError());
    if (!on_device) LPF_HIP(c, hipMemcpyAsync(inside, d_out, (size_t)k * B, hipMemcpyDeviceToHost, c->stream));
    LPF_HIP(c, host_wait(c));           // bp is a local
    return LPF_OK;
}

// OpenCV's weight table of one axis (resize.cpp: the xofs / alpha loop of resizeGeneric_, 8-bit INTER_LINEAR): per destination index
// {source index, second source index, w0, w1}.  Every step is a separate IEEE operation (volatile: no contraction, no excess precision).
// `clamp`: the x axis -- resize() sets {index, fraction} to {0, 0} / {n_src - 1, 0} beyond the ends.  The y axis keeps the fraction
// and only clips the two row indices (resizeGeneric_Invoker: clip(sy + k, 0, h)), so an edge row is blended with itself under both
// weights, whose two truncating shifts are not those of a single weight of 2048.
static void resize_table(int n_dst, int n_src, bool clamp, std::vector<int4> &tab)
{
    tab.resize((size_t)n_dst);
    volatile double ratio = (double)n_dst / (double)n_src;
    volatile double scale = 1.0 / ratio;
    for (int d = 0; d < n_dst; ++d) {
        volatile double a = ((double)d + 0.5) * scale;
        volatile double b = a - 0.5;
        volatile float f = (float)b;
        int s = (int)floorf(f);
        volatile float fr = f - (float)s;
        if (clamp && s < 0) { s = 0; fr = 0.f; }
        if (clamp && s >= n_src - 1) { s = n_src - 1; fr = 0.f; }
        volatile float one_minus = 1.0f - fr;
        volatile float p0 = one_minus * 2048.0f, p1 = fr * 2048.0f;
        long w0 = lrintf(p0), w1 = lrintf(p1);              // round half to even (the default rounding mode), as cvRound
        w0 = w0 < -32768 ? -32768 : w0 > 32767 ? 32767 : w0;
        w1 = w1 < -32768 ? -32768 : w1 > 32767 ? 32767 : w1;
        const int s0 = s < 0 ? 0 : s > n_src - 1 ? n_src - 1 : s, s1 = s + 1 < 0 ? 0 : s + 1 > n_src - 1 ? n_src - 1 : s + 1;
        tab[(size_t)d] = make_int4(s0, s1, (int)w0, (int)w1);
    }
}

// n planes [h][w] of uint8 -> n planes at the camera's size [H][W], as cv2.resize(plane, (W, H)) does (INTER_LINEAR; V3:222).
int lpf_resize_masks_u8(lpf_ctx *c, const uint8_t *src, int n, int h, int w, uint8_t *dst, int on_device)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (!c->have_camera) return fail(c, LPF_ERR_STATE, "lpf_set_camera has not been called (the target size is the camera's)");
    if (n < 0 || h <= 0 || w <= 0 || (n > 0 && (!src || !dst)) || (long long)h * w > 0x7fffffffll || (long long)n * h * w > (1ll << 36) ||
        (long long)n * c->W * c->H > (1ll << 36))
        return fail(c, LPF_ERR_ARG, "resize_masks: n=%d h=%d w=%d src=%p dst=%p (a plane of at most 2^31 - 1 pixels -- the kernel indexes it with "
                                    "32-bit arithmetic -- and at most 2^36 pixels in all, in and out)", n, h, w, (const void *)src, (void *)dst);
    if (n == 0) return LPF_OK;
    const int W = c->W, H = c->H;
    const bool area2 = w == 2 * W && h == 2 * H;              // cv2.resize hands this one to INTER_AREA: the rounded mean of 2 x 2 pixels
    const size_t in_bytes = (size_t)n * h * w, out_bytes = (size_t)n * H * W;
    int rc;
    if (c->capturing) return fail(c, LPF_ERR_STATE, "resize_masks inside a graph capture");
    if (c->pipe.owes() && (rc = sync_all(c))) return rc;                 // (the staging buffers below may be in use by owed runs)
    const uint8_t *dS = src;
    uint8_t *dD = dst;
    const bool linear = !area2 && !(h == H && w == W);
    std::vector<int4> xt, yt;
    const size_t tab_bytes = ((size_t)W + (size_t)H) * sizeof(int4);
    if ((rc = reserve(c, c->resize_buf, tab_bytes + (on_device ? 0 : in_bytes + out_bytes)))) return rc;
    if (linear) {
        resize_table(W, w, true, xt);
        resize_table(H, h, false, yt);
        // the tables are host vectors of this call: they travel through the pinned ring (copied now, queued in stream order), so a
        // device-mode call returns without waiting for the GPU
        if ((rc = upload(c, c->resize_buf.p, xt.data(), (size_t)W * sizeof(int4)))) return rc;
        if ((rc = upload(c, (char *)c->resize_buf.p + (size_t)W * sizeof(int4), yt.data(), (size_t)H * sizeof(int4)))) return rc;
    }
    if (!on_device) {
        dS = (const uint8_t *)c->resize_buf.p + tab_bytes;
        dD = (uint8_t *)c->resize_buf.p + tab_bytes + in_bytes;
        LPF_HIP(c, hipMemcpyAsync((void *)dS, src, in_bytes, hipMemcpyHostToDevice, c->stream));
    }
    if (!linear && !area2) {
        LPF_HIP(c, hipMemcpyAsync(dD, dS, out_bytes, hipMemcpyDeviceToDevice, c->stream));       // cv2.resize to the same size copies
    } else if (area2) {
        const long long quads = (long long)n * H * ((W + 3) / 4);
        hipLaunchKernelGGL(lpf_resize_area2_u8_kernel, dim3((unsigned)((quads + LPF_BLOCK - 1) / LPF_BLOCK)), dim3(LPF_BLOCK), 0, c->stream,
                           dS, dD, W, H, quads);
        LPF_HIP(c, hipGetLastError());
    } else {
        const long long total = (long long)out_bytes;
        hipLaunchKernelGGL(lpf_resize_linear_u8_kernel, dim3((unsigned)((total + LPF_BLOCK - 1) / LPF_BLOCK)), dim3(LPF_BLOCK), 0, c->stream,
                           dS, dD, (const int4 *)c->resize_buf.p, (const int4 *)c->resize_buf.p + W, w, h, W, H, total);
        LPF_HIP(c, hipGetLastError());
    }
    if (!on_device) {
        LPF_HIP(c, hipMemcpyAsync(dst, dD, out_bytes, hipMemcpyDeviceToHost, c->stream));
        LPF_HIP(c, host_wait(c));
    }
    return LPF_OK;
}

// n planes [h][w] of uint8 values, eroded `iters` times with the context's element (the 3x3 cross unless lpf_set_erosion_element says otherwise) at their own size (V3:83-90): see include/lpf.h
int lpf_erode_masks_u8(lpf_ctx *c, const uint8_t *src, int n, int h, int w, int iters, uint8_t *dst, int on_device)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (n < 0 || h <= 0 || w <= 0 || iters < 0 || (n > 0 && (!src || !dst || src == dst)) || (long long)h * w > 0x7fffffffll || (long long)n * h * w > (1ll << 36))
        return fail(c, LPF_ERR_ARG, "erode_masks: n=%d h=%d w=%d iters=%d src=%p dst=%p (src != dst)", n, h, w, iters, (const void *)src, (void *)dst);
    if (n == 0) return LPF_OK;
    if (c->capturing) return fail(c, LPF_ERR_STATE, "erode_masks inside a graph capture");
    int rc;
    if (c->pipe.owes() && (rc = sync_all(c))) return rc;                 // (the staging buffer below may be in use by owed runs)
    const size_t bytes = (size_t)n * h * w;
    // device callers: dst and one scratch plane set ping-pong; host callers: three staging copies
    if ((rc = reserve(c, c->resize_buf, on_device ? bytes : 3 * bytes))) return rc;
    uint8_t *a = on_device ? dst : (uint8_t *)c->resize_buf.p, *b = on_device ? (uint8_t *)c->resize_buf.p : (uint8_t *)c->resize_buf.p + bytes;
    const uint8_t *cur = src;
    if (!on_device) {
        uint8_t *in = (uint8_t *)c->resize_buf.p + 2 * bytes;
        LPF_HIP(c, hipMemcpyAsync(in, src, bytes, hipMemcpyHostToDevice, c->stream));
        cur = in;
    }
    const long long total = (long long)bytes;
    const dim3 g((unsigned)((total + LPF_BLOCK - 1) / LPF_BLOCK));
    // the last iteration must land in `a` (dst for device callers): with an even count the first one goes to b
    iters = erosion(c, iters).iters;                       // (the 1 x 1 element of lpf_set_erosion_element: the identity)
    uint8_t *out = (iters % 2 == 1) ? a : b;
    for (int it = 0; it < iters; ++it) {
        if (erosion(c, iters).element) hipLaunchKernelGGL(lpf_erode_u8_k_kernel, g, dim3(LPF_BLOCK), 0, c->stream, cur, out, w, h, total, c->erode_r, c->erode_spans);
        else hipLaunchKernelGGL(lpf_erode_u8_kernel, g, dim3(LPF_BLOCK), 0, c->stream, cur, out, w, h, total);
        LPF_HIP(c, hipGetLastError());
        cur = out;
        out = (out == a) ? b : a;
    }
    if (iters == 0) LPF_HIP(c, hipMemcpyAsync(a, cur, bytes, hipMemcpyDeviceToDevice, c->stream));
    if (!on_device) {
        LPF_HIP(c, hipMemcpyAsync(dst, a, bytes, hipMemcpyDeviceToHost, c->stream));
        LPF_HIP(c, host_wait(c));
    }
    return LPF_OK;
}

int lpf_depth_image(lpf_ctx *c, const float *pts, int64_t N, int on_device, double *depth_img, int32_t *winner)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (!c->have_camera) return fail(c, LPF_ERR_STATE, "lpf_set_camera has not been called");
    if (N < 0 || N > 0x7ffffff0ll || (N > 0 && !pts) || !depth_img) return fail(c, LPF_ERR_ARG, "depth_image: N=%lld", (long long)N);
    const size_t hw = (size_t)c->W * c->H;
    int rc;
    if ((rc = reserve(c, c->dimg, hw * 12))) return rc;                 // f64 image + u32 winners
    double *dD = on_device ? depth_img : (double *)c->dimg.p;
    unsigned *dW = (unsigned *)((char *)c->dimg.p + hw * 8);
    const float *dP = pts;
    if (!on_device && N > 0) {
        if ((rc = reserve(c, c->st_pts, (size_t)N * 16))) return rc;
        LPF_HIP(c, hipMemcpyAsync(c->st_pts.p, pts, (size_t)N * 16, hipMemcpyHostToDevice, c->stream));
        dP = (const float *)c->st_pts.p;
    }
    LPF_HIP(c, hipMemsetAsync(dD, 0, hw * 8, c->stream));
    LPF_HIP(c, hipMemsetAsync(dW, 0, hw * 4, c->stream));
    if (N > 0) {
        LpfCam P;
        set_cam(P, ctx_cam(c));
        const dim3 g((unsigned)((N + LPF_BLOCK - 1) / LPF_BLOCK));
        hipLaunchKernelGGL((lpf_depth_image_kernel<0>), g, dim3(LPF_BLOCK), 0, c->stream, P, (const float4 *)dP, (int)N, dW, dD);
        hipLaunchKernelGGL((lpf_depth_image_kernel<1>), g, dim3(LPF_BLOCK), 0, c->stream, P, (const float4 *)dP, (int)N, dW, dD);
        LPF_HIP(c, hipGetLastError());
    }
    if (!on_device) {
        LPF_HIP(c, hipMemcpyAsync(depth_img, dD, hw * 8, hipMemcpyDeviceToHost, c->stream));
        if (winner) {
            LPF_HIP(c, hipMemcpyAsync(winner, dW, hw * 4, hipMemcpyDeviceToHost, c->stream));
            LPF_HIP(c, host_wait(c));
            for (size_t i = 0; i < hw; ++i) winner[i] -= 1;          // stored as index + 1, 0 = none
            return LPF_OK;
        }
        LPF_HIP(c, host_wait(c));
    } else if (winner) {
        return fail(c, LPF_ERR_ARG, "depth_image: the winner image is only returned to host callers");
    }
    return LPF_OK;
}

int lpf_prepare_boxes(lpf_ctx *c, const double *corners_cam0, int nbox, const double Tcv[16], uint8_t *visible, double *corners_velo,
                      double *bbox2d, int32_t *front)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (!c->have_camera) return fail(c, LPF_ERR_STATE, "lpf_set_camera has not been called");
    if (nbox < 0 || (nbox > 0 && (!corners_cam0 || !Tcv))) return fail(c, LPF_ERR_ARG, "prepare_boxes: nbox=%d", nbox);
    if (nbox == 0) return LPF_OK;
    const size_t nb = (size_t)nbox;
    const size_t o_in = 0, o_cv = o_in + nb * 192, o_bb = o_cv + nb * 192, o_fr = o_bb + nb * 32, o_vis = o_fr + nb * 4, total = o_vis + nb;
    int rc;
    if (c->capturing) return fail(c, LPF_ERR_STATE, "prepare_boxes inside a graph capture");
    if ((rc = reserve(c, c->boxprep, total))) return rc;
    char *base = (char *)c->boxprep.p;
    // in through the pinned ring, back through a page-locked landing area in ONE copy (the four results lie behind each other): a
    // pageable pointer on either side makes every hipMemcpyAsync a blocking staged copy -- five of them were 0.9 ms per frame of
    // process_frames, fifty times the kernel
    if ((rc = upload(c, base + o_in, corners_cam0, nb * 192))) return rc;
    const size_t back = total - o_cv;
    if (c->pin_back.cap < back) {
        if (c->pin_back.p) { LPF_HIP(c, hipStreamSynchronize(c->stream)); (void)hipHostFree(c->pin_back.p); c->pin_back.p = nullptr; c->pin_back.cap = 0; }
        const size_t cap = back + back / 2 + 4096;
        LPF_HIP(c, hipHostMalloc((void **)&c->pin_back.p, cap, hipHostMallocDefault));
        c->pin_back.cap = cap;
    }
    LpfBoxPrep A;
    memcpy(A.Tcv, Tcv, sizeof A.Tcv);
    memcpy(A.K, c->K, sizeof A.K);
    A.W = c->W; A.H = c->H;
    hipLaunchKernelGGL(lpf_box_prep_kernel, dim3((unsigned)((nb * 8 + LPF_BLOCK - 1) / LPF_BLOCK)), dim3(LPF_BLOCK), 0, c->stream, A,
                       (const double *)(base + o_in), nbox, (uint8_t *)(base + o_vis), (double *)(base + o_cv), (double *)(base + o_bb),
                       (int *)(base + o_fr));
    LPF_HIP(c, hipGetLastError());
    LPF_HIP(c, hipMemcpyAsync(c->pin_back.p, base + o_cv, back, hipMemcpyDeviceToHost, c->stream));
    LPF_HIP(c, host_wait(c));
    const char *h = c->pin_back.p - o_cv;                         // (the landing area starts at the corners)
    if (visible) memcpy(visible, h + o_vis, nb);
    if (corners_velo) memcpy(corners_velo, h + o_cv, nb * 192);
    if (bbox2d) memcpy(bbox2d, h + o_bb, nb * 32);
    if (front) memcpy(front, h + o_fr, nb * 4);
    return LPF_OK;
}

int lpf_graph_begin(lpf_ctx *c)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (c->pipe.fused) return fail(c, LPF_ERR_STATE, "graph capture needs pipelining off");
    if (c->capturing) return fail(c, LPF_ERR_STATE, "already capturing");
    int rc = sync_all(c);
    if (rc) return rc;
    LPF_HIP(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    c->capturing = true;
    return LPF_OK;
}

int lpf_graph_end(lpf_ctx *c, lpf_graph **out)
{
    if (!c || !out) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (!c->capturing) return fail(c, LPF_ERR_STATE, "lpf_graph_end without lpf_graph_begin");
    { int rc_ = launch_box_job(c, c->boxes.in_force()); if (rc_) return rc_; }      // boxes set last in the capture, with no run behind them
    c->capturing = false;
    lpf_graph *g = new (std::nothrow) lpf_graph();
    if (!g) return fail(c, LPF_ERR_NOMEM, "out of host memory");
    hipError_t e = hipStreamEndCapture(c->stream, &g->graph);
    if (e == hipSuccess) e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        if (g->graph) (void)hipGraphDestroy(g->graph);
        delete g;
        return fail(c, LPF_ERR_HIP, "graph capture failed: %s (a call inside the capture allocated, copied from pageable memory or synchronised?)",
                    hipGetErrorString(e));
    }
    g->generation = c->generation;
    *out = g;
    return LPF_OK;
}

int lpf_graph_launch(lpf_ctx *c, lpf_graph *g)
{
    if (!c || !g || !g->exec) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (g->generation != c->generation)
        return fail(c, LPF_ERR_STATE, "lpf_graph_launch: the graph is stale -- since its capture the context changed geometry, boxes, camera, "
                                      "stream or mode, or regrew a buffer the graph points into; capture it again");
    LPF_HIP(c, hipGraphLaunch(g->exec, c->stream));
    return LPF_OK;
}

void lpf_graph_destroy(lpf_graph *g)
{
    if (!g) return;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
}

int lpf_get_stats(lpf_ctx *c, int64_t *out, int n, int reset)
{
    if (!c || (n > 0 && !out) || n < 0) return LPF_ERR_ARG;
    for (int i = 0; i < n; ++i) out[i] = i < 8 ? (int64_t)c->stats[i] : 0;
    if (reset) for (long long &v : c->stats) v = 0;
    return LPF_OK;
}

int lpf_profile_enable(lpf_ctx *c, int on)
{
    if (!c) return LPF_ERR_ARG;
    c->profiling = on != 0;
    return LPF_OK;
}

// ---- the one exchange step of the sharded path: a small int64 all-reduce over RCCL -----------------------
// librccl is resolved at the first call (dlopen), so liblpf.so carries no link-time dependency on it and a
// single-GPU user never loads it.  The communicator is the caller's (ncclCommInitRank / ncclCommInitAll).
int lpf_allreduce_metrics(lpf_ctx *c, int64_t *vec, int n, int op, void *rccl_comm)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (!vec || n <= 0 || n > (1 << 20) || op < 0 || op > 2 || !rccl_comm)
        return fail(c, LPF_ERR_ARG, "allreduce_metrics: vec=%p n=%d op=%d (0 sum, 1 min, 2 max) comm=%p", (void *)vec, n, op, rccl_comm);
    if (c->capturing) return fail(c, LPF_ERR_STATE, "lpf_allreduce_metrics inside graph capture");
    typedef int (*allreduce_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
    typedef const char *(*errstr_fn)(int);
    // The communicator belongs to whichever RCCL created it, and a process may hold more than one copy (torch wheels
    // bundle their own): take ncclAllReduce from a library that is ALREADY loaded -- the global scope first, then the
    // usual names without loading anything -- and only then load the system's librccl.  Resolved once (thread-safe).
    static allreduce_fn p_allreduce = nullptr;
    static errstr_fn p_errstr = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        void *h = nullptr;
        void *sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
        if (!sym) {
            for (const char *name : {"librccl.so", "librccl.so.1"}) {
                if ((h = dlopen(name, RTLD_NOW | RTLD_NOLOAD))) break;
            }
            if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
            if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (h) sym = dlsym(h, "ncclAllReduce");
        }
        p_allreduce = (allreduce_fn)sym;
        p_errstr = (errstr_fn)(h ? dlsym(h, "ncclGetErrorString") : dlsym(RTLD_DEFAULT, "ncclGetErrorString"));
    });
    if (!p_allreduce) return fail(c, LPF_ERR_STATE, "allreduce_metrics: no ncclAllReduce in this process and librccl.so cannot be loaded (%s)", dlerror());
    int rc;
    if ((rc = reserve(c, c->coll, (size_t)n * 8))) return rc;                 // a buffer of its own (lpf_points_in_boxes uses pib_out)
    LPF_HIP(c, hipMemcpyAsync(c->coll.p, vec, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    static const int red[3] = {0 /* ncclSum */, 3 /* ncclMin */, 2 /* ncclMax */};
    const int nrc = p_allreduce(c->coll.p, c->coll.p, (size_t)n, 4 /* ncclInt64 */, red[op], rccl_comm, c->stream);
    if (nrc != 0) return fail(c, LPF_ERR_HIP, "ncclAllReduce failed: %s", p_errstr ? p_errstr(nrc) : "?");
    LPF_HIP(c, hipMemcpyAsync(vec, c->coll.p, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    LPF_HIP(c, host_wait(c));          // blocks, with no timeout, until every rank has joined the collective
    return LPF_OK;
}

int lpf_profile_overhead(lpf_ctx *c, double *empty_bracket_ms)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    if (c->capturing) return fail(c, LPF_ERR_STATE, "lpf_profile_overhead inside graph capture");
    // What a pair of event records costs with nothing between them, on this stream, right now: the bracket
    // around a kernel contains this much that is not the kernel (median of 33 pairs, each after a sync).
    hipEvent_t e0, e1;
    LPF_HIP(c, hipEventCreate(&e0));
    LPF_HIP(c, hipEventCreate(&e1));
    float v[33];
    for (int i = 0; i < 33; ++i) {
        LPF_HIP(c, hipEventRecord(e0, c->stream));
        LPF_HIP(c, hipEventRecord(e1, c->stream));
        LPF_HIP(c, host_wait(c));
        LPF_HIP(c, hipEventElapsedTime(&v[i], e0, e1));
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    std::sort(v, v + 33);
    if (empty_bracket_ms) *empty_bracket_ms = (double)v[16];
    return LPF_OK;
}

int lpf_profile_read(lpf_ctx *c, double *k1_ms_sum, int64_t *k1_launches, int reset)
{
    if (!c) return LPF_ERR_ARG;
    if (use_device(c)) return LPF_ERR_HIP;
    LPF_HIP(c, host_wait(c));
    double sum = 0.0;
    for (size_t i = 0; i < c->ev_used; ++i) {
        float ms = 0.f;
        LPF_HIP(c, hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1]));
        sum += ms;
    }
    if (k1_ms_sum) *k1_ms_sum = sum;
    if (k1_launches) *k1_launches = (int64_t)c->ev_used;
    if (reset) c->ev_used = 0;
    return LPF_OK;
}

// ---- lpf_run_wide (include/lpf.h): frames of up to LPF_MAX_MASKS_WIDE masks, kernels in lpf_wide.hip.h ----------------------
// The parts of a wide run that lpf_run_cams_wide repeats per camera, on that camera's buffers D:

// The wide passes' label planes [F][LW][Himg][Wimg] (LW = ceil(M / 32) words per pixel, M > 0), in D's planes_a / planes_b; *planes =
// the buffer that holds the result.  Erosion runs on the packed planes, as F * LW images of uint32_t (erode_packed_iters).  From
// run-length masks: wide_pack_runs, above.  From dense masks in device memory [F][M][Himg][Wimg] (uint8, or float under `binarize`; rects: their rectangles where they hold,
// or NULL): the pack does the first erosion iteration itself, the remaining ones run on the planes
static int wide_pack_dense(lpf_ctx *c, lpf_ctx::Wide &D, const void *d_masks, const int4 *rects, bool f32, int binarize, int M, int erode_iters,
                           int F, int Wimg, int Himg, const uint32_t **planes)
{
    int rc;
    const int LW = (M + 31) / 32;
    if ((rc = reserve(c, D.planes_a, (size_t)F * LW * Wimg * Himg * 4))) return rc;
    uint32_t *cur = (uint32_t *)D.planes_a.p;
    const dim3 grid((Wimg + LPF_TW - 1) / LPF_TW, (Himg + LPF_TH - 1) / LPF_TH, (unsigned)(F * LW));
    const Erosion E = erosion(c, erode_iters);
    with_rule(f32, binarize + 1, [&](auto kind) {
        typedef typename decltype(kind)::elem T;
        if (E.element)                                    // the k x k element of lpf_set_erosion_element: its own kernels
            hipLaunchKernelGGL((lpf_wide_pack_k<T, decltype(kind)::rule>), grid, dim3(LPF_BLOCK), 0, c->stream, (const T *)d_masks, cur, M, LW, Himg, Wimg, c->erode_r, c->erode_spans);
        else
            hipLaunchKernelGGL((lpf_wide_pack<T, decltype(kind)::rule>), grid, dim3(LPF_BLOCK), 0, c->stream, (const T *)d_masks, cur, M, LW, Himg, Wimg, E.iters > 0 ? 1 : 0, rects);
    });
    LPF_HIP(c, hipGetLastError());
    if ((rc = erode_packed_iters(c, cur, D.planes_b, Wimg, Himg, F * LW, c->stream, E.iters - 1, E.element))) return rc;
    *planes = cur;
    return LPF_OK;
}

// Where a wide pass's label planes come from: M masks per frame, eroded erode_iters times, in exactly one of three forms, each checked
// by its pass before anything is enqueued
struct PlaneSource {
    int M, erode_iters;
    const lpf_wide_input *dense = nullptr;              // dense masks (check_wide_input)
    const lpf_ctx::RleIn *runs = nullptr;               // walked run-length masks (check_wide_rle)
    const lpf_id_masks *ids = nullptr;                  // instance-ID maps (check_ids)
    // a pass's lpf_wide_input and what check_wide_rle made of it: R.in is NULL when its masks are dense
    PlaneSource(const lpf_wide_input &in, const lpf_ctx::RleIn &R)
        : M(in.M), erode_iters(in.erode_iters), dense(R.in ? nullptr : &in), runs(R.in ? &R : nullptr) {}
    explicit PlaneSource(const lpf_id_masks &in) : M(in.M), erode_iters(in.erode_iters), ids(&in) {}
};

// ... from a pass's PlaneSource: dense host masks are staged into D and *host_in is set, device masks are lent; runs and ID maps are
// decoded (wide_pack_runs, wide_pack_ids).  *planes = NULL without masks
static int wide_pack(lpf_ctx *c, lpf_ctx::Wide &D, const PlaneSource &src, int F, int Wimg, int Himg, const uint32_t **planes, bool *host_in)
{
    *planes = nullptr;
    if (src.M == 0) return LPF_OK;
    if (src.ids) return wide_pack_ids(c, D, src.ids, Wimg, Himg, planes, host_in);
    if (src.runs) return wide_pack_runs(c, D, *src.runs, Wimg, Himg, planes, host_in);
    int rc;
    const lpf_wide_input &in = *src.dense;
    const void *d_masks = nullptr;
    const int4 *rects = nullptr;
    if ((rc = stage_masks(c, in, F, (size_t)Wimg * Himg, D.masks, D.rects, &d_masks, &rects, host_in))) return rc;
    return wide_pack_dense(c, D, d_masks, rects, in.f32 != 0, in.binarize, src.M, src.erode_iters, F, Wimg, Himg, planes);
}

// outputs and scratch of a wide run of n points, F frames, W.M masks, Btot boxes, W.nchunk chunks, on buffers D -> W's pointers: the
// caller's device pointers, or pieces of D.out (Stage; S.back(c) queues a host caller's copies)
static int wide_bind(lpf_ctx *c, lpf_ctx::Wide &D, const lpf_wide_outputs *out, size_t n, int F, int Btot, LpfWideParams &W, Stage &S)
{
    int rc;
    const int M = W.M, LW = W.LW, nchunk = W.nchunk;
    const size_t nF = (size_t)F, nFM = (size_t)F * M, nMB = (size_t)M * Btot, ncap = out->inst_cap > 0 ? (size_t)F * out->inst_cap : 0;
    // every output field of lpf_wide_outputs is bound here and nowhere else (uv and the label words: the later stages read them)
    S.host = !out->on_device;
    S.add(W.uv, out->uv, 8, n, true);
    S.add(W.depth, out->depth, 8, n);
    S.add(W.uf, out->u_f, 8, n);
    S.add(W.vf, out->v_f, 8, n);
    S.add(W.valid_idx, out->valid_idx, 8, n);
    S.add(W.uv_valid, out->uv_valid, 8, n);
    S.add(W.label_words, out->label_words, 4, n * LW, true);
    S.add(W.label_valid, out->label_valid_words, 4, n * LW);
    S.add(W.inst_idx, out->inst_idx, 8, ncap);
    S.add(W.count_out, out->count_mb, 4, nMB);
    S.add(W.n_valid, out->n_valid, 8, nF);
    S.add(W.n_labelled, out->n_labelled, 8, nF);
    S.add(W.inst_count, out->inst_count, 8, nFM);
    S.add(W.inst_off, out->inst_off, 8, nFM + nF);
    S.add(W.best_cnt, out->best_cnt, 8, nFM);
    S.add(W.best_box, out->best_box, 4, nFM);
    S.add(W.inst_overflow, out->inst_overflow, 4, nF);
    if ((rc = S.commit(c, D.out))) return rc;
    if ((rc = reserve(c, D.flags, (size_t)std::max(nchunk, 1) * LPF_WIDE_CHUNK))) return rc;
    if ((rc = reserve(c, D.ccnt, (size_t)std::max(nchunk, 1) * 8))) return rc;
    if ((rc = reserve(c, D.cpre, (size_t)std::max(nchunk, 1) * 8))) return rc;
    if ((rc = reserve(c, D.fcnt, nF * 8))) return rc;
    if ((rc = reserve(c, D.midx, n * 4))) return rc;
    if ((rc = reserve(c, D.mwords, n * LW * 4))) return rc;
    if ((rc = reserve(c, D.mpts, n * 16))) return rc;
    if ((rc = reserve(c, D.cnt, nMB * 4))) return rc;
    W.flags = (uint32_t *)D.flags.p; W.chunk_cnt = (int2 *)D.ccnt.p; W.chunk_pre = (int2 *)D.cpre.p; W.fcnt = (int2 *)D.fcnt.p;
    W.m_idx = (int *)D.midx.p; W.m_words = (uint32_t *)D.mwords.p; W.m_pts = (float4 *)D.mpts.p; W.cnt = (unsigned *)D.cnt.p;
    return LPF_OK;
}

// lpf_run_wide's run, behind the checks of the call's arguments, frames and masks (src: where the label planes come from).  who: the
// messages' prefix.  direct: the projecting stage reads the lent uint8 masks inside their rectangles (lpf_wide_direct_project) instead
// of packing them into planes for lpf_wide_project -- lpf_run_frame_wide's form for sparse frames; the caller has checked that
// src.dense's masks / rects are device memory, uint8, no erosion, M > 0, rects 16-byte aligned.  Everything else is shared: the box job,
// the frame table, wide_bind and the launches after projection.
static int run_wide_impl(lpf_ctx *c, const char *who, const float *pts, const int64_t *frame_off, int F, int pts_on_device,
                         const PlaneSource &src, const lpf_wide_outputs *out, bool direct)
{
    int rc;
    const int M = src.M;
    const int64_t Ntot = frame_off[F];
    if (out->inst_idx && out->inst_cap <= 0) return fail(c, LPF_ERR_ARG, "%s: inst_idx given with inst_cap=%lld", who, (long long)out->inst_cap);
    lpf_ctx::BoxSet &BX = c->boxes.in_force();
    if (BX.F != 0 && BX.F != F) return fail(c, LPF_ERR_STATE, "boxes were set for %d frames, %s has %d", BX.F, who, F);
    // a software-pipelined context launches what it owes first (no host wait): everything below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;
    c->boxes.claimed_by_run();
    if ((rc = launch_box_job(c, BX))) return rc;

    const int LW = (M + 31) / 32;
    const int Btot = BX.total();
    const bool host_io = !out->on_device;
    const size_t n = (size_t)Ntot;
    lpf_ctx::Wide &D = c->wide;

    // frame table
    std::vector<LpfWideFrame> fr((size_t)F);
    int nbw = 0;
    const int nchunk = wide_frames(frame_off, F, BX, fr.data(), &nbw);
    if ((rc = reserve(c, D.tab, (size_t)F * sizeof(LpfWideFrame)))) return rc;
    if ((rc = upload(c, D.tab.p, fr.data(), (size_t)F * sizeof(LpfWideFrame)))) return rc;

    LpfWideParams W;
    wide_params(W, ctx_cam(c), F, M, nchunk, nbw, BX, out->inst_cap, (const LpfWideFrame *)D.tab.p);

    // inputs: points, masks (host masks are staged; device masks are lent), rectangles
    bool pts_in = false, masks_in = false;
    if ((rc = host_points(c, D.pts, pts, pts_on_device != 0, 0, n, n, &W.pts, &pts_in))) return rc;
    if (direct) W.planes = nullptr;
    else if ((rc = wide_pack(c, D, src, F, c->W, c->H, &W.planes, &masks_in))) return rc;

    // ---- buffers: the caller's device pointers, or staging for host callers ---------------------------------------------------
    const size_t nMB = (size_t)M * Btot;
    Stage S;
    if ((rc = wide_bind(c, D, out, n, F, Btot, W, S))) return rc;

    // ---- the launch set ------------------------------------------------------------------------------------------------------
    if (nchunk > 0) {
        if (direct)
            hipLaunchKernelGGL(lpf_wide_direct_project, dim3((unsigned)nchunk), dim3(LPF_BLOCK), 0, c->stream, W, (const uint8_t *)src.dense->masks,
                               (const int4 *)src.dense->rects);
        else
            hipLaunchKernelGGL(lpf_wide_project, dim3((unsigned)nchunk), dim3(LPF_BLOCK), 0, c->stream, W);
        LPF_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(lpf_wide_scan, dim3((unsigned)F), dim3(LPF_BLOCK), 0, c->stream, W);
    LPF_HIP(c, hipGetLastError());
    if (nchunk > 0) {
        hipLaunchKernelGGL(lpf_wide_scatter, dim3((unsigned)nchunk), dim3(LPF_BLOCK), 0, c->stream, W);
        LPF_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(lpf_wide_lists, dim3((unsigned)(F * std::max(LW, 1))), dim3(LPF_BLOCK), 0, c->stream, W);
    LPF_HIP(c, hipGetLastError());
    if (M > 0) {
        if (nMB > 0) {
            LPF_HIP(c, hipMemsetAsync(D.cnt.p, 0, nMB * 4, c->stream));
            hipLaunchKernelGGL(lpf_wide_boxes, dim3((unsigned)(F * LW * W.nbw), LPF_WIDE_PARTS), dim3(LPF_BLOCK), 0, c->stream, W);
            LPF_HIP(c, hipGetLastError());
        }
        hipLaunchKernelGGL(lpf_wide_best, dim3((unsigned)F), dim3(LPF_BLOCK), 0, c->stream, W);
        LPF_HIP(c, hipGetLastError());
    }

    if (host_io && (rc = S.back(c))) return rc;
    if (host_io || masks_in || pts_in) LPF_HIP(c, host_wait(c));   // host buffers may be reused
    if (direct) ++c->stats[7];
    return LPF_OK;
}

// A wide run on a lpf_wide_input (lpf_run_wide, lpf_run_frame_wide): the checks -- run-length masks are checked in full here, into
// rle_in[0], before anything is enqueued -- then run_wide_impl
static int run_wide_input(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_wide_input *in,
                          const lpf_wide_outputs *out, bool direct)
{
    int rc;
    const char *who = "run_wide";
    if ((rc = enter(c, "lpf_run_wide", true))) return rc;
    if (!in || !out || !frame_off || F <= 0) return fail(c, LPF_ERR_ARG, "%s: in=%p out=%p frame_off=%p F=%d", who, (const void *)in, (const void *)out, (const void *)frame_off, F);
    if ((rc = check_wide_input(c, who, -1, *in, LPF_MAX_MASKS_WIDE, "lpf_run_wide takes 0 .. LPF_MAX_MASKS_WIDE", "", true))) return rc;
    if ((rc = check_frames(c, who, pts, frame_off, F, LPF_WIDE_CHUNK))) return rc;
    lpf_ctx::RleIn &R = c->rle_in[0];
    if ((rc = check_wide_rle(c, who, -1, *in, F, (long long)c->W * c->H, R))) return rc;
    return run_wide_impl(c, who, pts, frame_off, F, pts_on_device, PlaneSource(*in, R), out, direct);
}

int lpf_run_wide(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_wide_input *in,
                 const lpf_wide_outputs *out)
{
    return run_wide_input(c, pts, frame_off, F, pts_on_device, in, out, false);
}

// lpf_run_wide with its planes built from instance-ID maps: the struct is checked here, before run_wide_impl launches what a pipelined
// context owes or queues anything; the run itself is lpf_run_wide's, with wide_pack_ids as the source of its planes
int lpf_run_wide_ids(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_id_masks *in,
                     const lpf_wide_outputs *out)
{
    int rc;
    const char *who = "run_wide_ids";
    if ((rc = enter(c, "lpf_run_wide_ids", true))) return rc;
    if (!in) return fail(c, LPF_ERR_ARG, "run_wide_ids: in=NULL");
    if (in->M > LPF_MAX_MASKS_WIDE)
        return fail(c, LPF_ERR_ARG, "run_wide_ids: M=%d masks per frame, lpf_run_wide_ids takes 0 .. LPF_MAX_MASKS_WIDE = %d", in->M, LPF_MAX_MASKS_WIDE);
    if ((rc = check_ids(c, who, in, (size_t)c->W * c->H))) return rc;
    if (in->F != F) return fail(c, LPF_ERR_ARG, "run_wide_ids: the ID maps say F=%d, the call has F=%d", in->F, F);
    if (!out || !frame_off || F <= 0) return fail(c, LPF_ERR_ARG, "%s: in=%p out=%p frame_off=%p F=%d", who, (const void *)in, (const void *)out, (const void *)frame_off, F);
    if ((rc = check_frames(c, who, pts, frame_off, F, LPF_WIDE_CHUNK))) return rc;
    return run_wide_impl(c, who, pts, frame_off, F, pts_on_device, PlaneSource(*in), out, false);
}

// ---- lpf_depth_maps (include/lpf.h): per-car depth maps as sparse lists, kernels in lpf_depth_maps.hip.h ----------------------
// Frames go through in chunks of Fc (plan_ranges, the same cost for every frame): Fc winner planes, counters, staged masks / points
// (and label planes with erosion).

// lpf_dm_raster for the masks' element type and rule (or, with erosion, the planes packed from them): the count walk, or (scatter) the
// writing one
static void dm_raster(lpf_ctx *c, const LpfDmParams &P, dim3 g, bool planes, const lpf_wide_input *in, bool scatter)
{
    with_flag(scatter, [&](auto sc) {
        constexpr bool S = decltype(sc)::value;
        if (planes) hipLaunchKernelGGL((lpf_dm_raster<uint32_t, 0, true, S>), g, dim3(LPF_BLOCK), 0, c->stream, P);
        else with_rule(in->f32 != 0, in->binarize + 1, [&](auto kind) {
            hipLaunchKernelGGL((lpf_dm_raster<typename decltype(kind)::elem, decltype(kind)::rule, false, S>), g, dim3(LPF_BLOCK), 0, c->stream, P);
        });
    });
}

// What lpf_depth_maps and lpf_depth_maps_rle share, after the checks of their own mask input (who: the messages' prefix).  rle: the
// run-length masks of lpf_depth_maps_rle, not walked yet -- `in` then carries M and erode_iters only, and the label planes of a chunk are
// decoded from the chunk's own runs (RleCall::pack: wide_pack_runs on a lpf_ctx::RleSlice); NULL: the dense masks of `in`
static int depth_maps_impl(lpf_ctx *c, const char *who, const float *pts, const int64_t *frame_off, int F, int pts_on_device,
                           const lpf_wide_input *in, const lpf_rle_masks *rle, const lpf_depth_maps_outputs *out)
{
    int rc;
    const int M = in->M;
    if (out->cap < 0 || !out->car_off || !out->need || (out->cap > 0 && !out->pix))
        return fail(c, LPF_ERR_ARG, "%s: cap=%lld pix=%p car_off=%p need=%p (car_off and need are required, pix with cap > 0)", who,
                    (long long)out->cap, (void *)out->pix, (void *)out->car_off, (void *)out->need);
    if (F == 0) return LPF_OK;
    if ((rc = check_frames(c, who, pts, frame_off, F, LPF_BLOCK))) return rc;
    RleCall R(c);                                           // run-length masks: the whole batch checked here, before anything is enqueued
    if (rle && (rc = R.walk(who, rle, c->W, c->H))) return rc;
    const bool runs = R.active();
    long long maxN = 0;
    for (int f = 0; f < F; ++f) maxN = std::max(maxN, (long long)(frame_off[f + 1] - frame_off[f]));
    const int64_t Ntot = frame_off[F];
    // a software-pipelined context launches what it owes first (no host wait): everything below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;

    lpf_ctx::DepthMaps &D = c->dmaps;
    const size_t hw = (size_t)c->W * c->H, esz = in->f32 ? 4 : 1;
    const int ntile = (int)((hw + LPF_DM_TILE - 1) / LPF_DM_TILE), LW = (M + 31) / 32;
    const size_t hwp = (size_t)ntile * LPF_DM_TILE;
    const bool planes = M > 0 && (runs || in->erode_iters > 0);
    const bool host_masks = M > 0 && !runs && !in->on_device, host_pts = Ntot > 0 && !pts_on_device, host_io = !out->on_device;
    const bool use_rects = M > 0 && !runs && rects_hold(*in);
    // (decoded planes are eroded from the first iteration on, so they ping-pong with one iteration already; packed ones with two)
    const size_t plane_sets = in->erode_iters > (runs ? 0 : 1) ? 2 : 1;
    const size_t per_frame = hwp * 4 + (size_t)M * ntile * 12 + (planes ? (size_t)LW * hw * 4 * plane_sets : 0) +
                             (host_masks ? (size_t)M * (hw * esz + 16) : 0) + (host_pts ? (size_t)maxN * 16 : 0);
    const std::vector<Span> chunks = plan_ranges(c, (size_t)F, (size_t)F, [&](size_t f0, size_t n) {
        return n * per_frame + R.bytes(f0, n);                // (a chunk's run tables in place of its dense masks)
    });
    const size_t Fc = largest(chunks, [](size_t, size_t n) { return n; });      // (the first chunk's, where every frame costs the same)
    const size_t most_pts = largest(chunks, [&](size_t f0, size_t n) { return frame_off[f0 + n] - frame_off[f0]; });

    // ---- buffers, reserved for the largest chunk ------------------------------------------------------------------------------------
    if ((rc = reserve(c, D.foff, (size_t)(F + 1) * 8))) return rc;
    if ((rc = reserve(c, D.win, Fc * hwp * 4))) return rc;
    if (M > 0 && (rc = reserve(c, D.cnt, Fc * M * (2 * ntile + 1) * 4))) return rc;
    if (host_pts && (rc = reserve(c, D.pts, most_pts * 16))) return rc;      // (here, not by the first chunk with points: no chunk waits)
    if (runs && (rc = R.reserve_ranges(D.pack, chunks))) return rc;
    const void *masks_k = nullptr;                            // a chunk's staged masks and rectangles, or the caller's
    const int32_t *rects_k = nullptr;
    Stage I(host_masks);
    I.add(masks_k, M > 0 && !runs ? in->masks : nullptr, (size_t)M * hw * esz, Fc);
    I.add(rects_k, M > 0 && !runs ? in->rects : nullptr, (size_t)M * 16, Fc);
    if ((rc = I.commit(c, D.in))) return rc;
    const size_t cap = (size_t)out->cap, nF = (size_t)F;
    if ((rc = upload(c, D.foff.p, frame_off, (size_t)(F + 1) * 8))) return rc;

    LpfDmParams P;
    memset(&P, 0, sizeof P);
    set_cam(P.cam, ctx_cam(c));
    P.M = M; P.LW = LW; P.ntile = ntile; P.hwp = (long long)hwp; P.cap = out->cap;
    P.foff = (const long long *)D.foff.p;
    P.win = (unsigned *)D.win.p;
    P.cnt = (unsigned *)D.cnt.p;
    P.toff = P.cnt + Fc * M * ntile;
    P.tot = P.toff + Fc * M * ntile;
    // the whole batch's outputs (a host caller's lists only with room in them: cap > 0)
    const bool lists = cap > 0 || !host_io;
    Stage S(host_io);
    S.add(P.pix, lists ? out->pix : nullptr, 8, nF * cap);
    S.add(P.depth, lists ? out->depth : nullptr, 8, nF * cap);
    S.add(P.pidx, lists ? out->point_idx : nullptr, 8, nF * cap);
    S.add(P.car_off, out->car_off, 8, nF * (M + 1));
    S.add(P.need, out->need, 8, nF);
    S.add(P.overflow, out->overflow, 4, nF);
    if ((rc = S.commit(c, D.out))) return rc;

    // ---- the chunks ---------------------------------------------------------------------------------------------------------
    bool pts_in = false, runs_in = false;
    for (size_t k = 0; k < chunks.size(); ++k) {
        const Span &ch = chunks[k];
        const int f0 = (int)ch.first, fc = (int)ch.count;
        const long long a = frame_off[f0], nc = frame_off[f0 + fc] - a;
        long long mc = 0;
        for (int f = f0; f < f0 + fc; ++f) mc = std::max(mc, (long long)(frame_off[f + 1] - frame_off[f]));
        P.f0 = f0; P.pt_base = a;
        if ((rc = host_points(c, D.pts, pts, pts_on_device != 0, (size_t)a, (size_t)nc, most_pts, &P.pts, &pts_in))) return rc;
        if (nc == 0) P.pts = nullptr;
        if (M > 0) {
            if ((rc = I.in(c, {{ch.first, ch.count}, {ch.first, ch.count}}))) return rc;             // masks | rects
            const void *dm = host_masks || runs ? masks_k : (const char *)masks_k + ch.first * M * hw * esz;
            const int32_t *dr = host_masks || !rects_k ? rects_k : rects_k + ch.first * M * 4;
            P.masks = dm;
            P.rects = use_rects ? (const int4 *)dr : nullptr;
            const uint32_t *packed = nullptr;
            // the chunk's own runs: zeroed planes, decode, every erosion iteration; or, with erosion, lpf_run_wide's pack + erode into
            // LW planes per frame (no rectangles: they do not hold with erosion, rects_hold)
            if (runs) rc = R.pack(D.pack, k, &packed, &runs_in);
            else if (planes) rc = wide_pack_dense(c, D.pack, dm, nullptr, in->f32 != 0, in->binarize, M, in->erode_iters, fc, c->W, c->H, &packed);
            if (rc) return rc;
            if (planes) { P.masks = packed; P.rects = nullptr; }
            LPF_HIP(c, hipMemsetAsync(D.win.p, 0, (size_t)fc * hwp * 4, c->stream));
            LPF_HIP(c, hipMemsetAsync(D.cnt.p, 0, (size_t)fc * M * ntile * 4, c->stream));
            if (mc > 0) {
                hipLaunchKernelGGL(lpf_dm_winner, dim3((unsigned)((mc + LPF_BLOCK - 1) / LPF_BLOCK), (unsigned)fc), dim3(LPF_BLOCK), 0, c->stream, P);
                LPF_HIP(c, hipGetLastError());
                dm_raster(c, P, dim3((unsigned)((ntile + 3) / 4), (unsigned)fc, (unsigned)((M + LPF_DM_MGROUP - 1) / LPF_DM_MGROUP)), planes, in, false);
                LPF_HIP(c, hipGetLastError());
            }
            hipLaunchKernelGGL(lpf_dm_scan, dim3((unsigned)((M + 3) / 4), (unsigned)fc), dim3(LPF_BLOCK), 0, c->stream, P);
            LPF_HIP(c, hipGetLastError());
        }
        hipLaunchKernelGGL(lpf_dm_frame, dim3((unsigned)fc), dim3(LPF_BLOCK), 0, c->stream, P);
        LPF_HIP(c, hipGetLastError());
        if (M > 0 && mc > 0 && cap > 0) {
            dm_raster(c, P, dim3((unsigned)((ntile + 3) / 4), (unsigned)fc, (unsigned)((M + LPF_DM_MGROUP - 1) / LPF_DM_MGROUP)), planes, in, true);
            LPF_HIP(c, hipGetLastError());
        }
    }

    if (host_io && (rc = S.back(c))) return rc;
    if (host_io || host_masks || pts_in || runs_in) LPF_HIP(c, host_wait(c));   // host buffers may be reused
    return LPF_OK;                                            // (R lets go of the caller's arrays here: the copies have run)
}

int lpf_depth_maps(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_wide_input *in,
                   const lpf_depth_maps_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_depth_maps", true))) return rc;
    if (!in || !out || F < 0 || (F > 0 && !frame_off))
        return fail(c, LPF_ERR_ARG, "depth_maps: in=%p out=%p frame_off=%p F=%d", (const void *)in, (const void *)out, (const void *)frame_off, F);
    if ((rc = check_wide_input(c, "depth_maps", -1, *in, LPF_MAX_MASKS_WIDE, "lpf_depth_maps takes 0 .. LPF_MAX_MASKS_WIDE", ""))) return rc;
    return depth_maps_impl(c, "depth_maps", pts, frame_off, F, pts_on_device, in, nullptr, out);
}

int lpf_depth_maps_rle(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_rle_masks *masks,
                       const lpf_depth_maps_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_depth_maps_rle", true))) return rc;
    if (!masks || !out || F < 0 || (F > 0 && !frame_off))
        return fail(c, LPF_ERR_ARG, "depth_maps_rle: masks=%p out=%p frame_off=%p F=%d", (const void *)masks, (const void *)out,
                    (const void *)frame_off, F);
    if (masks->F != F) return fail(c, LPF_ERR_ARG, "depth_maps_rle: the run-length masks say F=%d, the call has F=%d", masks->F, F);
    if (masks->M < 0 || masks->M > LPF_MAX_MASKS_WIDE)
        return fail(c, LPF_ERR_ARG, "depth_maps_rle: M=%d masks per frame, lpf_depth_maps_rle takes 0 .. LPF_MAX_MASKS_WIDE = %d", masks->M,
                    LPF_MAX_MASKS_WIDE);
    if (masks->erode_iters < 0 || masks->reserved != 0)
        return fail(c, LPF_ERR_ARG, "depth_maps_rle: erode_iters=%d reserved=%d", masks->erode_iters, masks->reserved);
    lpf_wide_input in;                                      // M and erode_iters for the shared body; no dense masks behind it
    memset(&in, 0, sizeof in);
    in.M = masks->M; in.erode_iters = masks->erode_iters;
    return depth_maps_impl(c, "depth_maps_rle", pts, frame_off, F, pts_on_device, &in, masks, out);
}

// ---- lpf_depth_overlays (include/lpf.h): per-car overlay images, kernels in lpf_depth_overlays.hip.h -----------------------------
// The F * M (frame, car) images go through in chunks of consecutive images (plan_ranges): a chunk stages the segmented images and lists
// of the frames it touches when they are in host memory, its images when the outputs are.
#define LPF_DO_MAX_IMAGES 65535             // images per chunk: the render's grid.y

// host lists: offsets non-decreasing within [0, cap], pixels strictly ascending within each car and inside the image, depths finite
// and > 0 (the device lists are clamped by the kernels instead)
static int check_overlay_lists(lpf_ctx *c, int F, const lpf_depth_overlay_input *in, long long hw)
{
    const int M = in->M;
    const long long cap = in->cap;
    for (int f = 0; f < F; ++f) {
        const int64_t *off = in->car_off + (size_t)f * (M + 1);
        const int64_t *pix = in->pix ? in->pix + (size_t)f * cap : nullptr;
        const double *dep = in->depth ? in->depth + (size_t)f * cap : nullptr;
        if (off[0] < 0 || off[M] > cap)
            return fail(c, LPF_ERR_ARG, "depth_overlays: frame %d: car_off %lld .. %lld outside [0, cap = %lld]", f, (long long)off[0], (long long)off[M], cap);
        for (int m = 0; m < M; ++m) {
            if (off[m + 1] < off[m])
                return fail(c, LPF_ERR_ARG, "depth_overlays: frame %d: car_off decreases at car %d", f, m);
            for (int64_t e = off[m]; e < off[m + 1]; ++e) {
                if (pix[e] < 0 || pix[e] >= hw || (e > off[m] && pix[e] <= pix[e - 1]))
                    return fail(c, LPF_ERR_ARG, "depth_overlays: frame %d car %d: pixel %lld at entry %lld is outside the image or not ascending",
                                f, m, (long long)pix[e], (long long)e);
                if (!(std::isfinite(dep[e]) && dep[e] > 0.0))
                    return fail(c, LPF_ERR_ARG, "depth_overlays: frame %d car %d: depth %g at entry %lld is not finite and > 0", f, m, dep[e], (long long)e);
            }
        }
    }
    return LPF_OK;
}

int lpf_depth_overlays(lpf_ctx *c, int F, const lpf_depth_overlay_input *in, const lpf_depth_overlay_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_depth_overlays", true))) return rc;
    if (!in || !out || F < 0) return fail(c, LPF_ERR_ARG, "depth_overlays: in=%p out=%p F=%d", (const void *)in, (const void *)out, F);
    const int M = in->M;
    if (M < 0 || M > LPF_MAX_MASKS_WIDE)
        return fail(c, LPF_ERR_ARG, "depth_overlays: M=%d cars per frame, lpf_depth_overlays takes 0 .. LPF_MAX_MASKS_WIDE = %d", M, LPF_MAX_MASKS_WIDE);
    if (in->cap < 0 || !in->car_off || (M > 0 && !in->seg) || (in->cap > 0 && (!in->pix || !in->depth)))
        return fail(c, LPF_ERR_ARG, "depth_overlays: cap=%lld pix=%p depth=%p car_off=%p seg=%p (car_off is required, seg with M > 0, pix and depth with cap > 0)",
                    (long long)in->cap, (const void *)in->pix, (const void *)in->depth, (const void *)in->car_off, (const void *)in->seg);
    if (M > 0 && !out->images && !out->max_depth) return fail(c, LPF_ERR_ARG, "depth_overlays: images and max_depth are both NULL");
    const long long hw = (long long)c->W * c->H, cap = in->cap;
    if (!in->lists_on_device && F > 0 && (rc = check_overlay_lists(c, F, in, hw))) return rc;
    if (F == 0 || M == 0) return LPF_OK;
    // a software-pipelined context launches what it owes first (no host wait): everything below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;

    lpf_ctx::CallBufs &D = c->dovl;
    const size_t img_b = (size_t)hw * 3, total = (size_t)F * M;
    const bool host_seg = !in->seg_on_device, host_lists = !in->lists_on_device, host_out = !out->on_device;
    const bool want_img = out->images != nullptr, host_img = want_img && host_out, host_mx = out->max_depth && host_out;
    const size_t pix_b = (size_t)cap * 8, off_b = (size_t)(M + 1) * 8;
    const size_t per_image = host_img ? img_b : 0;
    const size_t per_frame = (host_seg ? img_b : 0) + (host_lists ? 2 * pix_b + off_b : 0);

    // ---- the chunks: [i0, i0 + n) of the F * M images, of frames [fa, fa + nf) ----------------------------------------------------
    auto frames_of = [&](size_t i0, size_t n) { return (i0 + n - 1) / M - i0 / M + 1; };
    const std::vector<Span> chunks = plan_ranges(c, total, LPF_DO_MAX_IMAGES, [&](size_t i0, size_t n) { return n * per_image + frames_of(i0, n) * per_frame; });
    const size_t most_img = largest(chunks, [](size_t, size_t n) { return n; }), most_fr = largest(chunks, frames_of);

    LpfDoParams Q;
    memset(&Q, 0, sizeof Q);
    Q.hw = hw; Q.M = M; Q.cap = cap;
    Stage I(host_seg);                                        // per frame: the segmented image; pixels, depths and offsets of the lists
    I.add(Q.seg, in->seg, img_b, most_fr);
    I.host = host_lists;
    I.add(Q.pix, in->pix, pix_b, most_fr);
    I.add(Q.depth, in->depth, pix_b, most_fr);
    I.add(Q.car_off, in->car_off, off_b, most_fr);
    if ((rc = I.commit(c, D.in))) return rc;
    unsigned char *img_k = nullptr;
    Stage O(host_out);                                        // a chunk's images; the batch's max_depth
    O.add(img_k, out->images, img_b, most_img);
    O.add(Q.mx, out->max_depth, 8, total);
    if ((rc = O.commit(c, D.out))) return rc;
    // pixels per render thread: 16 (three dwordx4) or 4 (three dwords) when that divides W * H and the bases allow it, else 1
    auto fits = [&](uintptr_t al) { return hw % (long long)al == 0 && ((uintptr_t)Q.seg % al) == 0 && ((uintptr_t)img_k % al) == 0; };
    const int P = fits(16) ? 16 : fits(4) ? 4 : 1;
    const unsigned gx = (unsigned)(((hw + P - 1) / P + LPF_BLOCK - 1) / LPF_BLOCK);
    for (const Span &ch : chunks) {
        const size_t i0 = ch.first, n = ch.count, fa = i0 / M, nf = frames_of(i0, n);
        Q.i0 = (long long)i0; Q.n = (long long)n;
        if ((rc = I.in(c, {{fa, nf}, {fa, nf}, {fa, nf}, {fa, nf}}))) return rc;                     // seg | pix | depth | car_off
        Q.seg_f0 = host_seg ? (long long)fa : 0;              // the staged arrays begin at the chunk's first frame
        Q.list_f0 = host_lists ? (long long)fa : 0;
        Q.img = want_img ? (host_img ? img_k : img_k + i0 * img_b) : nullptr;
        if (want_img) {
            const dim3 g(gx, (unsigned)n);
            if (P == 16) hipLaunchKernelGGL(lpf_do_render<16>, g, dim3(LPF_BLOCK), 0, c->stream, Q);
            else if (P == 4) hipLaunchKernelGGL(lpf_do_render<4>, g, dim3(LPF_BLOCK), 0, c->stream, Q);
            else hipLaunchKernelGGL(lpf_do_render<1>, g, dim3(LPF_BLOCK), 0, c->stream, Q);
            LPF_HIP(c, hipGetLastError());
        }
        hipLaunchKernelGGL(lpf_do_paint, dim3((unsigned)((n + 3) / 4)), dim3(LPF_BLOCK), 0, c->stream, Q);
        LPF_HIP(c, hipGetLastError());
        if ((rc = O.back(c, {{i0, n}, {0, 0}}))) return rc;                                       // images | max_depth
    }
    if ((rc = O.back(c, {{0, 0}, {0, total}}))) return rc;                                        // images | max_depth
    if (host_img || host_mx || host_seg || host_lists) LPF_HIP(c, host_wait(c));    // host buffers filled, or free to be reused
    return LPF_OK;
}

// ---- lpf_match_2d (include/lpf.h): V4 / V5 pair scoring of a batch, kernel in lpf_match2d.hip.h ---------------------------------------
// With every array in device memory the whole batch is one launch per 65535 frames on the caller's arrays.  Host arrays go through in
// ranges of consecutive frames (plan_ranges): a range stages its detections, rectangles and front counts when the inputs are in host
// memory, its best_box / best_iou rows and matrices when the outputs are.
#define LPF_M2_MAX_FRAMES 65535             // frames per launch: the grid's y

int lpf_match_2d(lpf_ctx *c, int F, const lpf_match2d_input *in, const lpf_match2d_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_match_2d", false))) return rc;
    if (!in || !out || F < 0) return fail(c, LPF_ERR_ARG, "match_2d: in=%p out=%p F=%d", (const void *)in, (const void *)out, F);
    if (!in->det_off || !in->box_off)
        return fail(c, LPF_ERR_ARG, "match_2d: det_off=%p box_off=%p (both are required, F + 1 entries each)", (const void *)in->det_off, (const void *)in->box_off);
    if (in->det_off[0] < 0 || in->box_off[0] < 0)
        return fail(c, LPF_ERR_ARG, "match_2d: det_off[0]=%d box_off[0]=%d (offsets start at 0 or above)", in->det_off[0], in->box_off[0]);
    if ((rc = check_m2_input(c, "match_2d", F, in, true, true))) return rc;
    double *const mats_out[5] = {out->iou, out->center_score, out->size_score, out->total_score, out->cost};
    int nmat = 0;
    for (double *m : mats_out) nmat += m != nullptr;
    const bool want_best = out->best_box || out->best_iou;
    if (F == 0 || in->det_off[F] == in->det_off[0] || (!want_best && !nmat)) return LPF_OK;
    // a software-pipelined context launches what it owes first (no host wait): everything below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;

    lpf_ctx::CallBufs &D = c->m2d;
    const bool host_in = !in->on_device, host_out = !out->on_device;
    const size_t esz = in->dets_f64 ? 8 : 4;

    // ---- the frame table and the ranges of frames: a frame stages its host inputs and host outputs --------------------------------------
    const M2Plan P = m2_plan(c, in->det_off, in->box_off, F, LPF_M2_MAX_FRAMES, [&](const LpfM2Frame &t) {
        return (host_in ? (size_t)t.D * 4 * esz + (size_t)t.B * 36 : 0) + (host_out ? (size_t)t.D * 12 + (size_t)nmat * 8 * (size_t)t.D * (size_t)t.B : 0);
    });
    if ((rc = upload_table(c, D.tab, P.tab.data(), (size_t)F))) return rc;

    LpfM2Params Q;
    memset(&Q, 0, sizeof Q);
    Q.min_iou = in->min_iou; Q.w_iou = in->w_iou; Q.w_center = in->w_center; Q.w_size = in->w_size;
    Stage I(host_in), O(host_out);
    I.add(Q.dets, in->dets, 4 * esz, P.most_d);
    I.add(Q.bbox2d, in->bbox2d, 32, P.most_b);
    I.add(Q.front, in->front, 4, P.most_b);
    if ((rc = I.commit(c, D.in))) return rc;
    O.add(Q.best_box, out->best_box, 4, P.most_d);
    O.add(Q.best_iou, out->best_iou, 8, P.most_d);
    O.add(Q.iou, out->iou, 8, P.most_p);
    O.add(Q.center, out->center_score, 8, P.most_p);
    O.add(Q.size, out->size_score, 8, P.most_p);
    O.add(Q.total, out->total_score, 8, P.most_p);
    O.add(Q.cost, out->cost, 8, P.most_p);
    if ((rc = O.commit(c, D.out))) return rc;
    const bool scores = out->center_score || out->size_score || out->total_score || out->cost;
    for (const M2Range &R : P.ranges) {
        if (R.most_rows == 0) continue;                     // no detections in the range: nothing to write
        Q.frames = (const LpfM2Frame *)D.tab.p + R.fa;
        if ((rc = I.in(c, {{R.d0, R.nd}, {R.b0, R.nb}, {R.b0, R.nb}}))) return rc;                   // dets | bbox2d | front
        Q.det_base = range_base(host_in, (int)R.d0); Q.box_base = range_base(host_in, (int)R.b0);
        Q.det_out_base = range_base(host_out, (int)R.d0); Q.pair_base = range_base(host_out, (long long)R.p0);
        const dim3 g((unsigned)((R.most_rows + LPF_M2_ROWS - 1) / LPF_M2_ROWS), (unsigned)R.nf);
        if (in->dets_f64) {
            if (scores) hipLaunchKernelGGL((lpf_m2_pairs<double, true>), g, dim3(LPF_BLOCK), 0, c->stream, Q);
            else hipLaunchKernelGGL((lpf_m2_pairs<double, false>), g, dim3(LPF_BLOCK), 0, c->stream, Q);
        } else {
            if (scores) hipLaunchKernelGGL((lpf_m2_pairs<float, true>), g, dim3(LPF_BLOCK), 0, c->stream, Q);
            else hipLaunchKernelGGL((lpf_m2_pairs<float, false>), g, dim3(LPF_BLOCK), 0, c->stream, Q);
        }
        LPF_HIP(c, hipGetLastError());
        // best_box | best_iou | iou | center | size | total | cost
        const Span dets = {R.d0, R.nd}, pairs = {R.p0, R.np};
        if ((rc = O.back(c, {dets, dets, pairs, pairs, pairs, pairs, pairs}))) return rc;
    }
    if (host_in || host_out) LPF_HIP(c, host_wait(c));       // host outputs filled, host inputs free to be reused
    return LPF_OK;
}

// ---- lpf_assign_costs / lpf_assign_2d (include/lpf.h): V5's Hungarian assignment of a batch, kernels in lpf_assign.hip.h ----------------
// Both calls are one routine: frames go through in ranges of consecutive frames (plan_ranges) whose scratch -- the matrices of live
// columns, the live-column maps -- and staged host arrays stay within the budget; a range is three launches (pack, solve, and for
// lpf_assign_2d finish) behind a memset of its status.  m2 != NULL: lpf_assign_2d (the cost is scored from m2's detections and boxes).
#define LPF_AS_MAX_FRAMES 65535             // frames per launch: the pack grid's y
static_assert(LPF_AS_CAP == LPF_ASSIGN_MAX, "the kernels' cap is the header's");

static int assign_batch(lpf_ctx *c, const char *who, int F, const int32_t *det_off, const int32_t *box_off, const double *cost_in,
                        const lpf_match2d_input *m2, const int32_t *front, bool host_in, const lpf_assign2d_params *prm, int32_t *col_out,
                        int32_t *status_out, const lpf_assign2d_outputs *o2, bool host_out)
{
    int rc;
    if (!det_off || !box_off)
        return fail(c, LPF_ERR_ARG, "%s: det_off=%p box_off=%p (both are required, F + 1 entries each)", who, (const void *)det_off, (const void *)box_off);
    if ((rc = check_offsets(c, who, "det_off", det_off, F)) || (rc = check_offsets(c, who, "box_off", box_off, F))) return rc;
    if (F == 0) return LPF_OK;
    const size_t esz = m2 && m2->dets_f64 ? 8 : 4;

    for (int f = 0; f < F; ++f) {
        const int rows = det_off[f + 1] - det_off[f], cols = box_off[f + 1] - box_off[f];
        int live = cols;                                      // (columns in device memory are not counted here: all of them may be live)
        if (front && host_in) live = (int)std::count_if(front + box_off[f], front + box_off[f + 1], [](int32_t v) { return v > 0; });
        if (rows > LPF_ASSIGN_MAX || live > LPF_ASSIGN_MAX)
            return fail(c, LPF_ERR_ARG, "%s: frame %d: %d rows and %d live columns, a frame takes at most LPF_ASSIGN_MAX = %d of either", who, f,
                        rows, live, LPF_ASSIGN_MAX);
    }
    // ---- the frame table and the ranges of frames: a frame's scratch, its staged host inputs, its outputs ------------------------------
    const M2Plan P = m2_plan(c, det_off, box_off, F, LPF_AS_MAX_FRAMES, [&](const LpfM2Frame &t) {
        const size_t pairs = (size_t)t.D * (size_t)t.B, staged = m2 ? (size_t)t.D * 4 * esz + (size_t)t.B * 36 : pairs * 8 + (size_t)t.B * 4;
        return pairs * 8 + (size_t)t.B * 4 + 4 + (host_in ? staged : 0) + (size_t)t.D * (m2 ? 40 : 4) + 4;
    });
    const long long pairs = P.tab[(size_t)F].p0;
    if (!m2 && pairs > 0 && !cost_in) return fail(c, LPF_ERR_ARG, "%s: cost=%p with %lld pairs (required with pairs)", who, (const void *)cost_in, pairs);
    // a software-pipelined context launches what it owes first (no host wait): everything below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;

    lpf_ctx::CallBufs &D = c->asgn;
    if ((rc = upload_table(c, D.tab, P.tab.data(), (size_t)F))) return rc;

    LpfAsParams Q;
    memset(&Q, 0, sizeof Q);
    if (m2) { Q.w_iou = m2->w_iou; Q.w_center = m2->w_center; Q.w_size = m2->w_size; Q.min_score = prm->min_score_threshold; Q.min_iou = prm->min_iou_threshold; }
    Stage I(host_in), S(false), O(host_out);
    I.add(Q.cost, m2 ? nullptr : cost_in, 8, P.most_p);
    I.add(Q.dets, m2 ? m2->dets : nullptr, 4 * esz, P.most_d);
    I.add(Q.bbox2d, m2 ? m2->bbox2d : nullptr, 32, P.most_b);
    I.add(Q.front, front, 4, P.most_b);
    if ((rc = I.commit(c, D.in))) return rc;
    S.add(Q.scratch, nullptr, 8, P.most_p, true);
    S.add(Q.colmap, nullptr, 4, P.most_b, true);
    S.add(Q.nlive, nullptr, 4, P.most_f, true);
    if ((rc = S.commit(c, D.pts))) return rc;
    O.add(Q.col, col_out, 4, P.most_d, true);                  // (the call needs both itself)
    O.add(Q.status, status_out, 4, P.most_f, true);
    O.add(Q.iou, o2 ? o2->iou : nullptr, 8, P.most_d);
    O.add(Q.center, o2 ? o2->center_score : nullptr, 8, P.most_d);
    O.add(Q.size, o2 ? o2->size_score : nullptr, 8, P.most_d);
    O.add(Q.total, o2 ? o2->total_score : nullptr, 8, P.most_d);
    O.add(Q.accepted, o2 ? o2->accepted : nullptr, 4, P.most_d);
    if ((rc = O.commit(c, D.out))) return rc;
    const bool col_staged = host_out || !col_out, status_staged = host_out || !status_out;
    int *const status0 = Q.status;
    const bool finish = m2 && (Q.iou || Q.center || Q.size || Q.total || Q.accepted);
    for (const M2Range &R : P.ranges) {
        const Span dets = {R.d0, R.nd}, boxes = {R.b0, R.nb};
        Q.frames = (const LpfM2Frame *)D.tab.p + R.fa;
        if ((rc = I.in(c, {{R.p0, R.np}, dets, boxes, boxes}))) return rc;                           // cost | dets | bbox2d | front
        Q.det_base = range_base(host_in, (int)R.d0); Q.box_base = range_base(host_in, (int)R.b0); Q.pair_base = range_base(host_in, (long long)R.p0);
        Q.scr_pair_base = (long long)R.p0; Q.scr_box_base = (int)R.b0;                               // (the scratch is the range's own)
        Q.col_base = range_base(col_staged, (int)R.d0); Q.score_base = range_base(host_out, (int)R.d0);
        Q.status = status0 + (status_staged ? 0 : R.fa);      // (a pointer, not a base: the caller's own array is entered at the range's first frame)
        LPF_HIP(c, hipMemsetAsync(Q.status, 0, R.nf * 4, c->stream));
        const dim3 g((unsigned)std::max((R.most_rows + LPF_M2_ROWS - 1) / LPF_M2_ROWS, 1), (unsigned)R.nf);
        if (!m2) hipLaunchKernelGGL((lpf_as_pack<0>), g, dim3(LPF_BLOCK), 0, c->stream, Q);
        else if (m2->dets_f64) hipLaunchKernelGGL((lpf_as_pack<2>), g, dim3(LPF_BLOCK), 0, c->stream, Q);
        else hipLaunchKernelGGL((lpf_as_pack<1>), g, dim3(LPF_BLOCK), 0, c->stream, Q);
        LPF_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(lpf_as_solve, dim3((unsigned)R.nf), dim3(64), 0, c->stream, Q);
        LPF_HIP(c, hipGetLastError());
        if (finish) {
            if (m2->dets_f64) hipLaunchKernelGGL((lpf_as_finish<double>), dim3((unsigned)R.nf), dim3(LPF_BLOCK), 0, c->stream, Q);
            else hipLaunchKernelGGL((lpf_as_finish<float>), dim3((unsigned)R.nf), dim3(LPF_BLOCK), 0, c->stream, Q);
            LPF_HIP(c, hipGetLastError());
        }
        // col | status | iou | center | size | total | accepted
        if ((rc = O.back(c, {dets, {R.fa, R.nf}, dets, dets, dets, dets, dets}))) return rc;
    }
    if (host_in || host_out) LPF_HIP(c, host_wait(c));       // host outputs filled, host inputs free to be reused
    return LPF_OK;
}

int lpf_assign_costs(lpf_ctx *c, int F, const lpf_assign_input *in, const lpf_assign_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_assign_costs", false))) return rc;
    if (!in || !out || F < 0) return fail(c, LPF_ERR_ARG, "assign_costs: in=%p out=%p F=%d", (const void *)in, (const void *)out, F);
    return assign_batch(c, "assign_costs", F, in->det_off, in->box_off, in->cost, nullptr, in->front, !in->on_device, nullptr, out->col_of_row,
                        out->status, nullptr, !out->on_device);
}

int lpf_assign_2d(lpf_ctx *c, int F, const lpf_match2d_input *in, const lpf_assign2d_params *p, const lpf_assign2d_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_assign_2d", false))) return rc;
    if (!in || !p || !out || F < 0)
        return fail(c, LPF_ERR_ARG, "assign_2d: in=%p p=%p out=%p F=%d", (const void *)in, (const void *)p, (const void *)out, F);
    if ((rc = check_m2_input(c, "assign_2d", F, in, in->det_off && in->box_off && F > 0, false))) return rc;   // (the rest is assign_batch's to refuse)
    if (std::isnan(p->min_score_threshold) || std::isnan(p->min_iou_threshold))
        return fail(c, LPF_ERR_ARG, "assign_2d: min_score_threshold=%g min_iou_threshold=%g must be numbers", p->min_score_threshold, p->min_iou_threshold);
    return assign_batch(c, "assign_2d", F, in->det_off, in->box_off, nullptr, in, in->front, !in->on_device, p, out->box_of_det, out->status, out,
                        !out->on_device);
}

// ---- lpf_inside_masks (include/lpf.h): V3's inside / outside split of every car of a batch, kernel in lpf_inside.hip.h -----------------
// One launch per 65535 frames on the box parameters in force.  Host arrays are staged whole: the points, the four list arrays in one
// buffer, the five outputs in another; of the staged [F][inst_cap] outputs only what the kernel wrote -- the first inst_off[f][M] entries
// of a frame whose lists fitted -- goes back to the caller, so the rest of the caller's rows stays as it was.
#define LPF_IN_MAX_FRAMES 65535             // frames per launch: the grid's y

int lpf_inside_masks(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_inside_input *in,
                     const lpf_inside_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_inside_masks", false))) return rc;
    if (!in || !out || F < 0 || !frame_off)
        return fail(c, LPF_ERR_ARG, "inside_masks: in=%p out=%p frame_off=%p F=%d", (const void *)in, (const void *)out, (const void *)frame_off, F);
    const int M = in->M;
    if (M < 0 || M > LPF_MAX_MASKS_WIDE)
        return fail(c, LPF_ERR_ARG, "inside_masks: M=%d cars per frame, lpf_inside_masks takes 0 .. LPF_MAX_MASKS_WIDE = %d", M, LPF_MAX_MASKS_WIDE);
    if (in->inst_cap < 0 || in->min_points < 0)
        return fail(c, LPF_ERR_ARG, "inside_masks: inst_cap=%lld min_points=%d (neither may be negative)", (long long)in->inst_cap, in->min_points);
    if (F == 0) return LPF_OK;
    const long long cap = in->inst_cap;
    if (!in->inst_off || (M > 0 && (!in->best_box || !in->best_cnt || (cap > 0 && !in->inst_idx))))
        return fail(c, LPF_ERR_ARG, "inside_masks: inst_idx=%p inst_off=%p best_box=%p best_cnt=%p (inst_off is required, best_box and best_cnt with M > 0, inst_idx with inst_cap > 0)",
                    (const void *)in->inst_idx, (const void *)in->inst_off, (const void *)in->best_box, (const void *)in->best_cnt);
    if ((rc = check_frames(c, "inside_masks", pts, frame_off, F, 0))) return rc;
    lpf_ctx::BoxSet *in_force;
    if ((rc = boxes_in_force(c, "inside_masks", F, &in_force))) return rc;
    const lpf_ctx::BoxSet &BX = *in_force;
    const bool host_in = !in->on_device, host_out = !out->on_device;
    const size_t M1 = (size_t)M + 1;
    if (host_in) {
        for (int f = 0; f < F; ++f) {
            const int64_t *off = in->inst_off + (size_t)f * M1;
            if (off[0] < 0) return fail(c, LPF_ERR_ARG, "inside_masks: frame %d: inst_off[0]=%lld is negative", f, (long long)off[0]);
            const int B = BX.box_off[f + 1] - BX.box_off[f];
            for (int m = 0; m < M; ++m) {
                if (off[m + 1] < off[m]) return fail(c, LPF_ERR_ARG, "inside_masks: frame %d: inst_off decreases at car %d", f, m);
                const int32_t bb = in->best_box[(size_t)f * M + m];
                if (bb >= B) return fail(c, LPF_ERR_ARG, "inside_masks: frame %d car %d: best_box=%d, the frame has %d boxes", f, m, bb, B);
                if (in->best_cnt[(size_t)f * M + m] < 0)
                    return fail(c, LPF_ERR_ARG, "inside_masks: frame %d car %d: best_cnt=%lld is negative", f, m, (long long)in->best_cnt[(size_t)f * M + m]);
            }
        }
    }
    if (M == 0) return LPF_OK;
    // a software-pipelined context launches what it owes first (no host wait) -- the box tables of the set in force among it: everything
    // below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;

    lpf_ctx::CallBufs &D = c->insd;
    const size_t fc = (size_t)F * (size_t)cap, fm = (size_t)F * M, Ntot = (size_t)frame_off[F];
    // the offsets on the host: the copies back to a host caller are sized by them
    std::vector<int64_t> fetched;
    const int64_t *off_h = host_in ? in->inst_off : nullptr;
    const bool lists_back = host_out && cap > 0 && (out->inside || out->part_idx || out->part_xyz);
    if (!host_in && lists_back) {
        fetched.resize((size_t)F * M1);
        LPF_HIP(c, hipMemcpyAsync(fetched.data(), in->inst_off, fetched.size() * 8, hipMemcpyDeviceToHost, c->stream));
        LPF_HIP(c, host_wait(c));
        off_h = fetched.data();
    }

    if ((rc = upload_batch_frames(c, D.tab, frame_off, F, BX))) return rc;

    LpfInParams Q;
    memset(&Q, 0, sizeof Q);
    Q.frames = (const LpfBatchFrame *)D.tab.p;
    Q.inst_cap = cap; Q.M = M; Q.min_points = in->min_points;
    Q.boxp = (const double *)BX.boxp.p;
    bool pts_in = false;
    if ((rc = host_points(c, D.pts, pts, pts_on_device != 0, 0, Ntot, Ntot, &Q.pts, &pts_in))) return rc;
    Stage I(host_in), O(host_out);
    I.add(Q.inst_idx, in->inst_idx, 8, fc);
    I.add(Q.inst_off, in->inst_off, 8, (size_t)F * M1);
    I.add(Q.best_cnt, in->best_cnt, 8, fm);
    I.add(Q.best_box, in->best_box, 4, fm);
    if ((rc = I.commit(c, D.in)) || (rc = I.in(c))) return rc;
    O.add(Q.inside, out->inside, 1, fc);
    O.add(Q.part_idx, out->part_idx, 8, fc);
    O.add(Q.part_xyz, out->part_xyz, 12, fc);
    O.add(Q.n_inside, out->n_inside, 8, fm);
    O.add(Q.matched, out->matched, 4, fm);
    if ((rc = O.commit(c, D.out))) return rc;
    if (Q.inside || Q.part_idx || Q.part_xyz || Q.n_inside || Q.matched) {
        const int per_launch = (int)most_of(c, LPF_IN_MAX_FRAMES);
        note_ranges(c, ((size_t)F + per_launch - 1) / per_launch);
        for (int f0 = 0; f0 < F; f0 += per_launch) {
            Q.f0 = f0;
            const dim3 g((unsigned)M, (unsigned)std::min(F - f0, per_launch));
            with_flag(BX.oriented != 0, [&](auto oriented) {
                hipLaunchKernelGGL((lpf_inside_cars<decltype(oriented)::value>), g, dim3(LPF_BLOCK), 0, c->stream, Q);
            });
            LPF_HIP(c, hipGetLastError());
        }
    }
    if (host_out) {
        // the summaries whole; of the staged [F][inst_cap] rows only what the kernel wrote
        if ((rc = O.back(c, {{0, 0}, {0, 0}, {0, 0}, {0, fm}, {0, fm}}))) return rc;             // inside | part_idx | part_xyz | n_inside | matched
        for (int f = 0; lists_back && f < F; ++f) {
            const int64_t *off = off_h + (size_t)f * M1;
            const long long n = off[M];
            if (n <= 0 || n > cap) continue;                              // nothing listed, or lists that did not fit: the row is left alone
            const size_t r = (size_t)f * (size_t)cap;
            if (Q.inside) LPF_HIP(c, hipMemcpyAsync(out->inside + r, Q.inside + r, (size_t)n, hipMemcpyDeviceToHost, c->stream));
            if (Q.part_idx) LPF_HIP(c, hipMemcpyAsync(out->part_idx + r, Q.part_idx + r, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
            if (Q.part_xyz) LPF_HIP(c, hipMemcpyAsync(out->part_xyz + r * 3, Q.part_xyz + r * 3, (size_t)n * 12, hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (host_out || host_in || pts_in) LPF_HIP(c, host_wait(c));    // host outputs filled, host inputs free to be reused
    return LPF_OK;
}

// ---- lpf_box_points (include/lpf.h): per-box point counts, first boxes and point-level confusion counts, kernel in lpf_box_points.hip.h --
// One launch per 65535 frames on the box tables in force, into outputs zeroed in stream order.  Host arrays are staged whole: the points,
// the three list arrays in one buffer, the four outputs in another; of a staged first_box only the first n_valid[f] entries of a frame
// go back to a host caller, so the rest of the caller's array stays as it was (with lists in device memory the host does not know
// n_valid: the caller's first_box goes up first and comes back whole).
#define LPF_BP_MAX_FRAMES 65535             // frames per launch: the grid's y

int lpf_box_points(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_box_points_input *in,
                   const lpf_box_points_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_box_points", false))) return rc;
    if (!in || !out || F < 0 || !frame_off)
        return fail(c, LPF_ERR_ARG, "box_points: in=%p out=%p frame_off=%p F=%d", (const void *)in, (const void *)out, (const void *)frame_off, F);
    const int LW = in->LW;
    if (LW < 0 || LW > LPF_MAX_MASKS_WIDE / 32)
        return fail(c, LPF_ERR_ARG, "box_points: LW=%d label words per point, lpf_box_points takes 0 .. LPF_MAX_MASKS_WIDE / 32 = %d", LW,
                    LPF_MAX_MASKS_WIDE / 32);
    if (F == 0) return LPF_OK;
    if (!in->valid_idx || !in->n_valid)
        return fail(c, LPF_ERR_ARG, "box_points: valid_idx=%p n_valid=%p (both are required)", (const void *)in->valid_idx, (const void *)in->n_valid);
    if ((rc = check_frames(c, "box_points", pts, frame_off, F, 0))) return rc;
    lpf_ctx::BoxSet *in_force;
    if ((rc = boxes_in_force(c, "box_points", F, &in_force))) return rc;
    const lpf_ctx::BoxSet &BX = *in_force;
    const bool host_in = !in->on_device, host_out = !out->on_device;
    int64_t most = 0;                                       // entries of the frame with the most: the grid's x
    for (int f = 0; f < F; ++f) {
        const int64_t N = frame_off[f + 1] - frame_off[f];
        if (!host_in) { most = std::max(most, N); continue; }    // (lists in device memory: not known here; the kernel clamps n_valid to N)
        const int64_t n = in->n_valid[f];
        if (n < 0 || n > N) return fail(c, LPF_ERR_ARG, "box_points: frame %d: n_valid=%lld, the frame has %lld points", f, (long long)n, (long long)N);
        const int64_t *v = in->valid_idx + frame_off[f];
        for (int64_t e = 0; e < n; ++e) {
            if (v[e] < 0 || v[e] >= N)
                return fail(c, LPF_ERR_ARG, "box_points: frame %d entry %lld: index %lld, the frame has %lld points", f, (long long)e, (long long)v[e], (long long)N);
            if (e > 0 && v[e] <= v[e - 1])
                return fail(c, LPF_ERR_ARG, "box_points: frame %d entry %lld: index %lld does not ascend (the entry before is %lld)", f, (long long)e,
                            (long long)v[e], (long long)v[e - 1]);
        }
        most = std::max(most, n);
    }
    if (!out->box_points && !out->box_labelled && !out->first_box && !out->frame_counts) return LPF_OK;     // nothing is wanted
    // a software-pipelined context launches what it owes first (no host wait) -- the box tables of the set in force among it: everything
    // below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;

    lpf_ctx::CallBufs &D = c->bpts;
    const size_t Ntot = (size_t)frame_off[F], Btot = (size_t)BX.total();
    if ((rc = upload_batch_frames(c, D.tab, frame_off, F, BX))) return rc;

    LpfBpParams Q;
    memset(&Q, 0, sizeof Q);
    Q.frames = (const LpfBatchFrame *)D.tab.p;
    Q.boxp = (const double *)BX.boxp.p; Q.boxq = (const float *)BX.boxq.p;
    const bool labels = in->label_valid_words && LW > 0;
    Q.LW = labels ? LW : 0;
    bool pts_in = false;
    if ((rc = host_points(c, D.pts, pts, pts_on_device != 0, 0, Ntot, Ntot, &Q.pts, &pts_in))) return rc;
    Stage I(host_in), O(host_out);
    I.add(Q.valid_idx, in->valid_idx, 8, Ntot);
    I.add(Q.n_valid, in->n_valid, 8, (size_t)F);
    I.add(Q.labels, labels ? in->label_valid_words : nullptr, 4, Ntot * (size_t)LW);
    if ((rc = I.commit(c, D.in)) || (rc = I.in(c))) return rc;
    O.add(Q.box_points, out->box_points, 4, Btot);
    O.add(Q.box_labelled, out->box_labelled, 4, Btot);
    O.add(Q.first_box, out->first_box, 4, Ntot);
    O.add(Q.frame_counts, out->frame_counts, 32, (size_t)F);
    if ((rc = O.commit(c, D.out))) return rc;
    // the sums are added into zeroed outputs; a staged first_box whose written part the host cannot size starts as the caller's
    if (Q.box_points && Btot) LPF_HIP(c, hipMemsetAsync(Q.box_points, 0, Btot * 4, c->stream));
    if (Q.box_labelled && Btot) LPF_HIP(c, hipMemsetAsync(Q.box_labelled, 0, Btot * 4, c->stream));
    if (Q.frame_counts) LPF_HIP(c, hipMemsetAsync(Q.frame_counts, 0, (size_t)F * 32, c->stream));
    const bool first_whole = host_out && !host_in && out->first_box && Ntot;
    if (first_whole) LPF_HIP(c, hipMemcpyAsync(Q.first_box, out->first_box, Ntot * 4, hipMemcpyHostToDevice, c->stream));
    const unsigned gx = (unsigned)std::max<int64_t>((most + LPF_BP_CHUNK - 1) / LPF_BP_CHUNK, 1);     // (a block per frame writes frame_counts[f][0])
    const int per_launch = (int)most_of(c, LPF_BP_MAX_FRAMES);
    note_ranges(c, ((size_t)F + per_launch - 1) / per_launch);
    for (int f0 = 0; f0 < F; f0 += per_launch) {
        Q.f0 = f0;
        const dim3 g(gx, (unsigned)std::min(F - f0, per_launch));
        with_flag(BX.oriented != 0, [&](auto oriented) {
            hipLaunchKernelGGL((lpf_box_points_kernel<decltype(oriented)::value>), g, dim3(LPF_BLOCK), 0, c->stream, Q);
        });
        LPF_HIP(c, hipGetLastError());
    }
    if (host_out) {
        // box_points | box_labelled | first_box | frame_counts
        if ((rc = O.back(c, {{0, Btot}, {0, Btot}, {0, first_whole ? Ntot : 0}, {0, (size_t)F}}))) return rc;
        for (int f = 0; host_in && out->first_box && f < F; ++f) {
            const size_t n = (size_t)in->n_valid[f], r = (size_t)frame_off[f];
            if (n) LPF_HIP(c, hipMemcpyAsync(out->first_box + r, Q.first_box + r, n * 4, hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (host_out || host_in || pts_in) LPF_HIP(c, host_wait(c));    // host outputs filled, host inputs free to be reused
    return LPF_OK;
}

// ---- lpf_box_views (include/lpf.h): secondtest's view filter and V5's box projection of a batch, kernel in lpf_box_views.hip.h ----------
// With every array in device memory the whole batch is one launch on the caller's arrays, a block per frame.  Host arrays go through
// in ranges of consecutive frames (plan_ranges): a range stages its corners when the input is in host memory, its per-box outputs and
// frame counts when the outputs are.
int lpf_box_views(lpf_ctx *c, int F, const lpf_box_views_input *in, const lpf_box_views_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_box_views", true))) return rc;
    if (!in || !out || F < 0) return fail(c, LPF_ERR_ARG, "box_views: in=%p out=%p F=%d", (const void *)in, (const void *)out, F);
    if (!in->box_off) return fail(c, LPF_ERR_ARG, "box_views: box_off=%p (required, F + 1 entries)", (const void *)in->box_off);
    if ((rc = check_offsets(c, "box_views", "box_off", in->box_off, F))) return rc;
    if (in->box_off[F] > in->box_off[0] && !in->corners_cam0)
        return fail(c, LPF_ERR_ARG, "box_views: corners_cam0=%p with %d boxes (required with boxes)", (const void *)in->corners_cam0,
                    in->box_off[F] - in->box_off[0]);
    if (out->corners_velo && !in->T_cam_to_velo)
        return fail(c, LPF_ERR_ARG, "box_views: T_cam_to_velo=%p with corners_velo asked for (required for corners_velo)", (const void *)in->T_cam_to_velo);
    if (!std::isfinite(in->depth_lo) || !std::isfinite(in->depth_hi) || !std::isfinite(in->min_area))
        return fail(c, LPF_ERR_ARG, "box_views: depth_lo=%g depth_hi=%g min_area=%g must be finite", in->depth_lo, in->depth_hi, in->min_area);
    if (in->min_points_in_view < 0 || in->min_points_in_view > 8)
        return fail(c, LPF_ERR_ARG, "box_views: min_points_in_view=%d (0 .. 8: a box has 8 corners)", in->min_points_in_view);
    const void *const per_box[] = {out->keep, out->reason, out->corners_in_view, out->corners_near, out->avg_depth, out->near_bbox2d,
                                   out->front, out->bbox2d, out->front_avg_depth, out->kept_pos, out->corners_velo};
    const size_t per_box_esz[] = {1, 4, 4, 4, 8, 32, 4, 32, 8, 4, 192};
    size_t out_bytes = 0;                                    // of a box's wanted outputs
    bool any_box_out = false;
    for (int i = 0; i < 11; ++i)
        if (per_box[i]) { out_bytes += per_box_esz[i]; any_box_out = true; }
    if (F == 0 || (!any_box_out && !out->frame_counts)) return LPF_OK;
    // a software-pipelined context launches what it owes first (no host wait): everything below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;

    lpf_ctx::CallBufs &D = c->bviews;
    const bool host_in = !in->on_device, host_out = !out->on_device;

    // ---- the frame table and the ranges of frames; cost[f]: the bytes staged for the frames before f ---------------------------------
    std::vector<LpfBvFrame> tab((size_t)F);
    std::vector<size_t> cost((size_t)F + 1, 0);
    for (int f = 0; f < F; ++f) {
        LpfBvFrame &t = tab[(size_t)f];
        t.b0 = in->box_off[f]; t.B = in->box_off[f + 1] - t.b0;
        cost[(size_t)f + 1] = cost[(size_t)f] + (host_in ? (size_t)t.B * 192 : 0) + (host_out ? (size_t)t.B * out_bytes + 24 : 0);
    }
    const std::vector<Span> ranges = plan_ranges(c, (size_t)F, (size_t)F, [&](size_t f, size_t n) { return cost[f + n] - cost[f]; });
    const size_t most_b = largest(ranges, [&](size_t f, size_t n) { return in->box_off[f + n] - in->box_off[f]; });
    const size_t most_f = largest(ranges, [](size_t, size_t n) { return n; });
    if ((rc = upload_table(c, D.tab, tab.data(), (size_t)F))) return rc;

    LpfBvParams Q;
    memset(&Q, 0, sizeof Q);
    memcpy(Q.K, c->K, sizeof Q.K);
    if (in->T_cam_to_velo) memcpy(Q.Tcv, in->T_cam_to_velo, sizeof Q.Tcv);
    Q.W = c->W; Q.H = c->H; Q.min_in_view = in->min_points_in_view;
    Q.depth_lo = in->depth_lo; Q.depth_hi = in->depth_hi; Q.min_area = in->min_area;
    int *counts = nullptr;                                   // frame_counts of the range's first frame (staged) or of frame 0 (the caller's)
    Stage I(host_in), O(host_out);
    I.add(Q.corners, in->corners_cam0, 192, most_b);
    if ((rc = I.commit(c, D.in))) return rc;
    O.add(Q.keep, out->keep, 1, most_b);
    O.add(Q.reason, out->reason, 4, most_b);
    O.add(Q.in_view, out->corners_in_view, 4, most_b);
    O.add(Q.n_near, out->corners_near, 4, most_b);
    O.add(Q.avg_depth, out->avg_depth, 8, most_b);
    O.add(Q.near_bbox2d, out->near_bbox2d, 32, most_b);
    O.add(Q.front, out->front, 4, most_b);
    O.add(Q.bbox2d, out->bbox2d, 32, most_b);
    O.add(Q.front_avg_depth, out->front_avg_depth, 8, most_b);
    O.add(Q.kept_pos, out->kept_pos, 4, most_b);
    O.add(counts, out->frame_counts, 24, most_f);
    O.add(Q.corners_velo, out->corners_velo, 192, most_b);
    if ((rc = O.commit(c, D.out))) return rc;
    for (const Span &r : ranges) {
        const size_t fa = r.first, fb = fa + r.count;
        const size_t b0 = (size_t)in->box_off[fa], nb = (size_t)in->box_off[fb] - b0;
        if (nb == 0 && !counts) continue;                    // no boxes in the range and no counts to zero: nothing to write
        Q.frames = (const LpfBvFrame *)D.tab.p + fa;
        if ((rc = I.in(c, {{b0, nb}}))) return rc;
        // staged arrays begin at the range's first box and frame; the caller's own at the batch's
        Q.in_base = host_in ? (int)b0 : 0; Q.out_base = host_out ? (int)b0 : 0;
        Q.frame_counts = counts ? counts + (host_out ? 0 : fa * 6) : nullptr;
        hipLaunchKernelGGL(lpf_box_views_kernel, dim3((unsigned)r.count), dim3(LPF_BV_BLOCK), 0, c->stream, Q);
        LPF_HIP(c, hipGetLastError());
        // keep | reason | in_view | near | avg_depth | near_bbox2d | front | bbox2d | front_avg_depth | kept_pos | frame_counts | corners_velo
        if ((rc = O.back(c, {{b0, nb}, {b0, nb}, {b0, nb}, {b0, nb}, {b0, nb}, {b0, nb}, {b0, nb}, {b0, nb}, {b0, nb}, {b0, nb},
                             {fa, r.count}, {b0, nb}}))) return rc;
    }
    if (host_in || host_out) LPF_HIP(c, host_wait(c));       // host outputs filled, host inputs free to be reused
    return LPF_OK;
}

// ---- lpf_first_match (include/lpf.h): Same_color's first-mask labels of a batch, kernels in lpf_first_match.hip.h ---------------------
// Frames go through in ranges of consecutive frames (plan_ranges): a range stages its points, masks and colours when they are in host
// memory, its outputs when those are, and needs 4 bytes per point for the codes (unless the dense output takes them) plus 16 bytes per
// tile of 1024 points.  A host caller's lists go UP before the range's kernels and come back whole after them, as lpf_box_points does
// with a first_box it cannot size: what the kernels do not write -- a frame's span at or beyond its count -- returns as it was, and
// the call still ends with ONE host wait.
#define LPF_FM_MAX_FRAMES 65535             // frames per launch: the grid's y

// What lpf_first_match and lpf_first_match_rle share, after the checks of their own mask input (who: the messages' prefix).  rle: the
// run-length masks of lpf_first_match_rle, not walked yet -- `in` then carries M, mh, mw, the colours and where those are (on_device),
// a range's label planes [fc][LW][mh][mw] are decoded from the range's own runs (RleCall::pack: wide_pack_runs on a
// lpf_ctx::RleSlice) and lpf_fm_count_planes reads them; NULL: the dense masks of `in`
static int first_match_impl(lpf_ctx *c, const char *who, const float *pts, const int64_t *frame_off, int F, int pts_on_device,
                            const lpf_first_match_input *in, const lpf_rle_masks *rle, const lpf_first_match_outputs *out)
{
    int rc;
    const int M = in->M;
    if (out->car_rgb && !in->colors) return fail(c, LPF_ERR_ARG, "%s: car_rgb is asked for, colors is NULL", who);
    if (!out->n_car || !out->n_bg)
        return fail(c, LPF_ERR_ARG, "%s: n_car=%p n_bg=%p (both are required)", who, (void *)out->n_car, (void *)out->n_bg);
    if (F == 0) return LPF_OK;
    if ((rc = check_frames(c, who, pts, frame_off, F, LPF_FM_TILE))) return rc;
    RleCall R(c);                                           // run-length masks: the whole batch checked here, before anything is enqueued
    if (rle && (rc = R.walk(who, rle, M > 0 ? in->mw : 0, M > 0 ? in->mh : 0))) return rc;
    const bool runs = R.active();
    // a software-pipelined context launches what it owes first (no host wait): everything below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;

    lpf_ctx::FirstMatch &D = c->fmat;
    const size_t Ntot = (size_t)frame_off[F], nM = (size_t)M, LW = (nM + 31) / 32;
    const size_t plane = M > 0 ? (size_t)in->mh * (size_t)in->mw : 0, esz = in->f32 ? 4 : 1;
    // (host_masks: the range's masks AND colours are staged; with runs no mask is, and host_in says where the colours are)
    const bool host_masks = M > 0 && !runs && !in->on_device, host_in = M > 0 && !in->on_device;
    const bool host_pts = Ntot > 0 && !pts_on_device, host_io = !out->on_device;
    const bool dense = out->first_mask != nullptr;
    const bool lists = out->car_idx || out->car_mask || out->car_xyz || out->car_rgb || out->bg_idx || out->bg_xyz;
    auto given = [](const void *p, size_t b) { return p ? b : (size_t)0; };
    const size_t out_pt = given(out->first_mask, 4) + given(out->car_idx, 8) + given(out->car_mask, 4) + given(out->car_xyz, 12) +
                          given(out->car_rgb, 24) + given(out->bg_idx, 8) + given(out->bg_xyz, 12);
    const size_t per_pt = (host_pts ? 16 : 0) + (dense ? 0 : 4) + (host_io ? out_pt : 0);
    const size_t per_fr = 16 + (host_masks ? nM * plane * esz : 0) + (host_in ? given(in->colors, nM * 24) : 0) +
                          (runs ? LW * plane * 4 : 0) + (host_io ? 24 + nM * 8 : 0);
    auto pts_of = [&](size_t f0, size_t n) { return (size_t)(frame_off[f0 + n] - frame_off[f0]); };
    const std::vector<Span> ranges = plan_ranges(c, (size_t)F, LPF_FM_MAX_FRAMES, [&](size_t f0, size_t n) {
        return pts_of(f0, n) * per_pt + pts_of(f0, n) / LPF_FM_TILE * 16 + n * per_fr + R.bytes(f0, n);
    });
    const size_t most_pts = largest(ranges, pts_of), most_f = largest(ranges, [](size_t, size_t n) { return n; });

    // ---- buffers, reserved for the largest range -------------------------------------------------------------------------------------
    const size_t most_tiles = most_pts / LPF_FM_TILE + most_f;
    if ((rc = reserve(c, D.tab, (size_t)(F + 1) * 8))) return rc;
    if (!dense && (rc = reserve(c, D.code, most_pts * 4))) return rc;
    if ((rc = reserve(c, D.tiles, most_tiles * 16))) return rc;
    if (host_pts && (rc = reserve(c, D.pts, most_pts * 16))) return rc;       // (here, not by the first range with points: no range waits)
    if (runs && (rc = R.reserve_ranges(D.pack, ranges))) return rc;
    if ((rc = upload(c, D.tab.p, frame_off, (size_t)(F + 1) * 8))) return rc;

    LpfFmParams P;
    memset(&P, 0, sizeof P);
    set_cam(P.cam, ctx_cam(c));
    P.M = M; P.mh = in->mh; P.mw = in->mw;
    P.foff = (const long long *)D.tab.p;
    P.tcnt = (int2 *)D.tiles.p;
    P.tpre = P.tcnt + most_tiles;
    const char *masks_k = nullptr;                            // a range's staged masks and colours, or the caller's
    const double *colors_k = nullptr;
    Stage I(host_in);
    I.add(masks_k, M > 0 && !runs ? in->masks : nullptr, nM * plane * esz, most_f);
    I.add(colors_k, M > 0 ? in->colors : nullptr, nM * 24, most_f);
    if ((rc = I.commit(c, D.in))) return rc;
    // a host caller's outputs are staged range by range, a device caller's are written in place
    const size_t np = host_io ? most_pts : Ntot, nf = host_io ? most_f : (size_t)F;
    int *dense_k = nullptr;
    Stage S(host_io);
    S.add(dense_k, out->first_mask, 4, np);
    S.add(P.car_idx, out->car_idx, 8, np);
    S.add(P.car_mask, out->car_mask, 4, np);
    S.add(P.car_xyz, out->car_xyz, 12, np);
    S.add(P.car_rgb, out->car_rgb, 24, np);
    S.add(P.bg_idx, out->bg_idx, 8, np);
    S.add(P.bg_xyz, out->bg_xyz, 12, np);
    S.add(P.n_valid, out->n_valid, 8, nf);
    S.add(P.n_car, out->n_car, 8, nf);
    S.add(P.n_bg, out->n_bg, 8, nf);
    S.add(P.mask_count, out->mask_count, 8, nf * nM);
    if ((rc = S.commit(c, D.out))) return rc;

    // ---- the ranges -----------------------------------------------------------------------------------------------------------------
    bool pts_in = false, runs_in = false;
    for (size_t k = 0; k < ranges.size(); ++k) {
        const Span &r = ranges[k];
        const int f0 = (int)r.first, fc = (int)r.count;
        const long long a = frame_off[f0], nc = frame_off[f0 + fc] - a;
        long long mc = 0;                                     // points of the range's largest frame: the grid's x
        for (int f = f0; f < f0 + fc; ++f) mc = std::max(mc, (long long)(frame_off[f + 1] - frame_off[f]));
        P.f0 = f0; P.pt_base = a;
        P.out_base = range_base(host_io, a); P.fr_base = range_base(host_io, (long long)f0);
        P.code = dense ? dense_k : (int *)D.code.p;
        P.code_base = dense ? P.out_base : a;
        if ((rc = host_points(c, D.pts, pts, pts_on_device != 0, (size_t)a, (size_t)nc, most_pts, &P.pts, &pts_in))) return rc;
        if (nc == 0) P.pts = nullptr;
        if (M > 0) {
            if ((rc = I.in(c, {{r.first, r.count}, {r.first, r.count}}))) return rc;                 // masks | colors
            P.masks = host_masks || runs ? masks_k : masks_k + r.first * nM * plane * esz;
            P.colors = host_in || !colors_k ? colors_k : colors_k + r.first * nM * 3;
            const uint32_t *decoded = nullptr;                // the range's own runs: zeroed planes, then the decode
            if (runs && (rc = R.pack(D.pack, k, &decoded, &runs_in))) return rc;
            if (runs) P.masks = decoded;
        }
        const Span sp = {(size_t)a, (size_t)nc}, sf = {r.first, r.count}, none = {0, 0};
        // first_mask | car_idx | car_mask | car_xyz | car_rgb | bg_idx | bg_xyz | n_valid | n_car | n_bg | mask_count: the lists as the
        // caller has them
        if (host_io && lists && (rc = S.in(c, {none, sp, sp, sp, sp, sp, sp, none, none, none, none}))) return rc;
        if (P.mask_count && M > 0)
            LPF_HIP(c, hipMemsetAsync(P.mask_count + (size_t)(f0 - P.fr_base) * nM, 0, (size_t)fc * nM * 8, c->stream));
        const dim3 g((unsigned)((mc + LPF_FM_TILE - 1) / LPF_FM_TILE), (unsigned)fc);
        if (mc > 0) {
            if (rle) hipLaunchKernelGGL(lpf_fm_count_planes, g, dim3(LPF_BLOCK), 0, c->stream, P);
            else with_flag(in->f32 != 0, [&](auto f32) {
                typedef typename std::conditional<decltype(f32)::value, float, uint8_t>::type T;
                hipLaunchKernelGGL(lpf_fm_count<T>, g, dim3(LPF_BLOCK), 0, c->stream, P);
            });
            LPF_HIP(c, hipGetLastError());
        }
        hipLaunchKernelGGL(lpf_fm_scan, dim3((unsigned)fc), dim3(LPF_BLOCK), 0, c->stream, P);
        LPF_HIP(c, hipGetLastError());
        if (mc > 0 && lists) {
            hipLaunchKernelGGL(lpf_fm_scatter, g, dim3(LPF_BLOCK), 0, c->stream, P);
            LPF_HIP(c, hipGetLastError());
        }
        if (host_io && (rc = S.back(c, {sp, sp, sp, sp, sp, sp, sp, sf, sf, sf, {r.first * nM, r.count * nM}}))) return rc;
    }
    if (host_io || host_in || pts_in || runs_in) LPF_HIP(c, host_wait(c));   // host outputs filled, host inputs free to be reused
    return LPF_OK;                                            // (R lets go of the caller's arrays here: the copies have run)
}

int lpf_first_match(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_first_match_input *in,
                    const lpf_first_match_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_first_match", true))) return rc;
    if (!in || !out || F < 0 || !frame_off)
        return fail(c, LPF_ERR_ARG, "first_match: in=%p out=%p frame_off=%p F=%d", (const void *)in, (const void *)out, (const void *)frame_off, F);
    const int M = in->M;
    if (M < 0 || M > LPF_MAX_MASKS_WIDE)
        return fail(c, LPF_ERR_ARG, "first_match: M=%d masks per frame, lpf_first_match takes 0 .. LPF_MAX_MASKS_WIDE = %d", M, LPF_MAX_MASKS_WIDE);
    if (in->f32 != LPF_MASKS_U8 && in->f32 != LPF_MASKS_F32)
        return fail(c, LPF_ERR_ARG, "first_match: f32=%d (LPF_MASKS_U8 = 0 or LPF_MASKS_F32 = 1: lpf_first_match takes dense masks only)", in->f32);
    if (M > 0 && (!in->masks || in->mh <= 0 || in->mw <= 0))
        return fail(c, LPF_ERR_ARG, "first_match: masks=%p mh=%d mw=%d (with M > 0 masks is required and mh, mw are > 0)", in->masks, in->mh, in->mw);
    return first_match_impl(c, "first_match", pts, frame_off, F, pts_on_device, in, nullptr, out);
}

int lpf_first_match_rle(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device,
                        const lpf_first_match_rle_input *in, const lpf_first_match_outputs *out)
{
    int rc;
    if ((rc = enter(c, "lpf_first_match_rle", true))) return rc;
    if (!in || !in->masks || !out || F < 0 || !frame_off)
        return fail(c, LPF_ERR_ARG, "first_match_rle: in=%p masks=%p out=%p frame_off=%p F=%d", (const void *)in,
                    (const void *)(in ? in->masks : nullptr), (const void *)out, (const void *)frame_off, F);
    const lpf_rle_masks *masks = in->masks;
    const int M = masks->M;
    if (masks->F != F) return fail(c, LPF_ERR_ARG, "first_match_rle: the run-length masks say F=%d, the call has F=%d", masks->F, F);
    if (M < 0 || M > LPF_MAX_MASKS_WIDE)
        return fail(c, LPF_ERR_ARG, "first_match_rle: M=%d masks per frame, lpf_first_match_rle takes 0 .. LPF_MAX_MASKS_WIDE = %d", M,
                    LPF_MAX_MASKS_WIDE);
    if (masks->erode_iters != 0)
        return fail(c, LPF_ERR_ARG, "first_match_rle: erode_iters=%d (the first-mask labelling has no erosion: 0)", masks->erode_iters);
    if (in->reserved != 0 || masks->reserved != 0)
        return fail(c, LPF_ERR_ARG, "first_match_rle: reserved=%d, the masks' reserved=%d (both 0)", in->reserved, masks->reserved);
    if (M > 0 && (in->mh <= 0 || in->mw <= 0))
        return fail(c, LPF_ERR_ARG, "first_match_rle: mh=%d mw=%d (with M > 0 both are > 0)", in->mh, in->mw);
    lpf_first_match_input fin;                              // M, the masks' size and the colours for the shared body; no dense masks behind it
    memset(&fin, 0, sizeof fin);
    fin.colors = in->colors; fin.M = M; fin.mh = in->mh; fin.mw = in->mw; fin.on_device = in->colors_on_device;
    return first_match_impl(c, "first_match_rle", pts, frame_off, F, pts_on_device, &fin, masks, out);
}

// ---- lpf_run_cams (include/lpf.h): one scan in up to LPF_MAX_CAMS cameras, kernels in lpf_cams.hip.h ------------------------------
// The checks lpf_run_cams and lpf_run_cams_wide share (who: the call's name; frames of up to 0x7fffffff - slack points; 0 .. max_M masks
// per camera, takes / more: what the message says about the limit, check_wide_input), after what every batched call begins with (enter).
static int cams_check(lpf_ctx *c, const char *who, const float *pts, const int64_t *frame_off, int F, const lpf_cam_input *cams, int C,
                      const void *out, int64_t slack, int max_M, const char *takes, const char *more)
{
    const char *w = who + 4;                               // "run_cams..." in the messages
    int rc;
    if ((rc = enter(c, who, false))) return rc;
    if (C < 1 || C > LPF_MAX_CAMS) return fail(c, LPF_ERR_ARG, "%s: C=%d cameras, a pass takes 1 .. LPF_MAX_CAMS = %d", w, C, LPF_MAX_CAMS);
    if (!cams || !out || !frame_off || F <= 0)
        return fail(c, LPF_ERR_ARG, "%s: cams=%p out=%p frame_off=%p F=%d", w, (const void *)cams, out, (const void *)frame_off, F);
    if ((rc = check_frames(c, w, pts, frame_off, F, slack))) return rc;
    for (int k = 0; k < C; ++k) {
        const lpf_cam_input &I = cams[k];
        if (I.W <= 0 || I.H <= 0 || (long long)I.W * I.H > (1ll << 30))
            return fail(c, LPF_ERR_ARG, "%s: camera %d is %d x %d", w, k, I.W, I.H);
        if ((rc = check_wide_input(c, w, k, I.masks, max_M, takes, more, true))) return rc;
        if ((rc = check_wide_rle(c, w, k, I.masks, F, (long long)I.W * I.H, c->rle_in[k]))) return rc;
        if (I.corners_velo) {
            if (!I.box_off || I.box_off[0] != 0) return fail(c, LPF_ERR_ARG, "%s: camera %d: box_off must be given and start at 0", w, k);
            for (int f = 0; f < F; ++f)
                if (I.box_off[f + 1] < I.box_off[f]) return fail(c, LPF_ERR_ARG, "%s: camera %d: box_off not ascending at %d", w, k, f);
            if (I.boxes_on_device < 0 || I.boxes_on_device > 2) return fail(c, LPF_ERR_ARG, "%s: camera %d: boxes_on_device=%d", w, k, I.boxes_on_device);
        }
    }
    return LPF_OK;
}

// camera k's box tables of a multi-camera pass: lpf_run_cams' box set k, shaped for F frames and filled by a box job launched here
// in camera k's K, W, H (lpf_set_boxes_ex's tables for that camera); no corners: no boxes
static int cams_box_tables(lpf_ctx *c, const lpf_cam_input &I, int k, int F)
{
    int rc;
    lpf_ctx::BoxSet &B = c->cams.bx[k];
    B.clear();
    if (!I.corners_velo) return LPF_OK;
    if ((rc = box_shape(c, B, I.box_off, F, I.oriented))) return rc;
    const size_t nb = (size_t)B.total();
    if (nb == 0) return LPF_OK;
    const double *src;
    if ((rc = stage_corners(c, B, I.corners_velo, I.boxes_on_device, nb, &src))) { B.clear(); return rc; }
    B.new_job(src);
    return launch_box_job(c, B, I.K, I.W, I.H);
}

// Camera c runs as the narrow in-order run would -- the same segments, counters, tables and tail -- in scratch set c, with its own box
// tables (c->cams.bx[c]) and label images (c->cams.label_a[c]); the three launches after the packs and box jobs serve every camera.
static_assert(LPF_MAX_CAMS == LPF_MAX_CAMS_DEV && LPF_MAX_CAMS <= LPF_NSETS, "a scratch set per camera");

int lpf_run_cams(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_cam_input *cams, int C,
                 const lpf_outputs *out)
{
    int rc;
    if ((rc = cams_check(c, "lpf_run_cams", pts, frame_off, F, cams, C, out, LPF_SEG_QUANTUM, LPF_MAX_MASKS, "a pass takes 0 .. LPF_MAX_MASKS",
                         " per camera (more: lpf_run_wide for that camera)")))
        return rc;
    const int64_t Ntot = frame_off[F];
    for (int k = 0; k < C; ++k) {
        if (out[k].inst_idx && out[k].inst_cap <= 0) return fail(c, LPF_ERR_ARG, "run_cams: out[%d].inst_idx given with inst_cap=%lld", k, (long long)out[k].inst_cap);
        if ((out[k].uv_valid || out[k].label_valid) && !out[k].valid_idx)
            return fail(c, LPF_ERR_ARG, "run_cams: out[%d]: uv_valid / label_valid need valid_idx as well (they share its order)", k);
    }
    // a software-pipelined context launches what it owes first (no host wait): everything below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;
    const size_t n = (size_t)Ntot;
    bool host_in = false;

    // ---- points: read once by the streaming launch ----------------------------------------------------------------------------------
    const float4 *d_pts;
    if ((rc = host_points(c, c->cams.pts, pts, pts_on_device != 0, 0, n, n, &d_pts, &host_in))) return rc;

    // ---- per camera: box tables (the box job), masks -> label images (one element type for the pass) ------------------------------
    int lb_all = 1;
    for (int k = 0; k < C; ++k) { const int M = cams[k].masks.M; lb_all = std::max(lb_all, M <= 8 ? 1 : M <= 16 ? 2 : 4); }
    const void *label_img[LPF_MAX_CAMS] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < C; ++k) {
        const lpf_cam_input &I = cams[k];
        if ((rc = cams_box_tables(c, I, k, F))) return rc;
        const lpf_wide_input &m = I.masks;
        if (m.M == 0) continue;
        const size_t hw = (size_t)I.W * I.H;
        const lpf_ctx::RleIn &R = c->rle_in[k];
        if (R.in) {
            // run-length masks: lpf_set_masks_rle's zero + decode (+ erosion on the packed image) at the pass's element width, into
            // this camera's label image
            void *cur = nullptr;
            if ((rc = rle_label_image(c, c->cams.label_a[k], c->cams.label_b[k], c->cams.rle[k], R, I.W, I.H, lb_all, &cur, &host_in))) return rc;
            label_img[k] = cur;
            continue;
        }
        const void *d_masks = nullptr;
        const int4 *rects = nullptr;
        if ((rc = stage_masks(c, m, F, hw, c->cams.masks[k], c->cams.rects[k], &d_masks, &rects, &host_in))) return rc;
        if (I.W < 16) rects = nullptr;                     // (as lpf_set_masks_*: a group of 16 pixels of the pack spans at most two rows)
        if ((rc = reserve(c, c->cams.label_a[k], (size_t)F * hw * 4))) return rc;
        DevBuf &la = c->cams.label_a[k], &lb2 = c->cams.label_b[k];
        void *cur = nullptr;
        const int mode = m.f32 ? m.binarize + 1 : 0;
        rc = pack_masks(c, la, lb2, I.W, I.H, c->stream, d_masks, m.f32 != 0, mode, lb_all, F, m.M, m.erode_iters, &cur, rects);
        if (rc) return rc;
        label_img[k] = cur;
    }

    // ---- segmentation: as lpf_run_batch's in-order run (it depends on the points only) ---------------------------------------------
    const bool small = Ntot <= LPF_SMALL_LAUNCH;
    const int tile_pts = (small && Ntot <= 1792ll * 512) ? 512 : 1024;
    LpfCamsArgs A;
    memset(&A, 0, sizeof A);
    A.C = C;
    int nk1 = 0, max_tail = 0;
    NarrowLayout L;
    for (int k = 0; k < C; ++k) {
        const lpf_cam_input &I = cams[k];
        const lpf_ctx::BoxSet &BX = c->cams.bx[k];
        const lpf_outputs &o = out[k];
        const int M = I.masks.M;
        const int Btot = BX.total();
        narrow_layout(c, frame_off, F, BX, o.inst_cap, small, L);
        lpf_ctx::Scratch &S = c->sc[k];
        if ((rc = narrow_reserve(c, S, L, M, Btot))) return rc;
        if (M > 0 && (rc = reserve(c, S.mlist, n * 16))) return rc;
        // geometry tables in scratch set k (count blocks in one part), uploaded every pass
        if ((rc = narrow_tables(c, S, L, true))) return rc;

        LpfParams &P = A.P[k];
        narrow_params(P, c, input_cam(I), L, S, BX, M, o.inst_cap);
        P.label_img = M > 0 ? label_img[k] : nullptr;
        P.mlist = M > 0 ? (float4 *)S.mlist.p : nullptr;
        P.pts = d_pts;
        P.tile_pts = tile_pts;
        nk1 = L.nseg_total * (int)(L.seg_pts / tile_pts);      // (the same for every camera, as L.pre_scan)

        if ((rc = narrow_bind(c, c->cams.out[k], o, n, F, M, Btot, P))) return rc;
        const bool want_lists = o.valid_idx || o.inst_idx;
        A.ntail[k] = (P.count_boxes ? L.ncblk : 0) + (want_lists ? L.nblk : 0);
        max_tail = std::max(max_tail, A.ntail[k]);
    }

    // ---- the launch set: streaming tiles of every camera, then every camera's tail, then every camera's summaries --------------------
    if (nk1 > 0) {
        const dim3 g1((unsigned)nk1);
        with_label(lb_all, [&](auto lt) {
            typedef typename decltype(lt)::type LT;
            if (tile_pts == 512) hipLaunchKernelGGL((lpf_cams_stream<2, LT>), g1, dim3(LPF_BLOCK), 0, c->stream, A);
            else hipLaunchKernelGGL((lpf_cams_stream<4, LT>), g1, dim3(LPF_BLOCK), 0, c->stream, A);
        });
        LPF_HIP(c, hipGetLastError());
    }
    if (L.pre_scan && nk1 > 0)                                 // frames beyond 64 groups (16.7 M points): their prefixes, per camera
        for (int k = 0; k < C; ++k) {
            hipLaunchKernelGGL(lpf_scan_segments, dim3((unsigned)F), dim3(LPF_BLOCK), 0, c->stream, A.P[k]);
            LPF_HIP(c, hipGetLastError());
        }
    if (max_tail > 0) {
        const dim3 gt((unsigned)max_tail, (unsigned)C);
        if (L.pre_scan) hipLaunchKernelGGL((lpf_cams_tail<true>), gt, dim3(LPF_BLOCK), 0, c->stream, A);
        else hipLaunchKernelGGL((lpf_cams_tail<false>), gt, dim3(LPF_BLOCK), 0, c->stream, A);
        LPF_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(lpf_cams_finalize, dim3((unsigned)F, (unsigned)C), dim3(LPF_BLOCK), 0, c->stream, A);
    LPF_HIP(c, hipGetLastError());

    // ---- host outputs: the dense arrays; the compact ones and the summaries written into page-locked result buffers by
    //      lpf_results_to_host (as lpf_run_batch does), or else -- once the summaries are here -- the filled part of each list -------
    bool any_host = false, lists_later = false;
    bool later[LPF_MAX_CAMS] = {false, false, false, false};
    std::vector<lpf_frame_summary> hs((size_t)F * C);
    for (int k = 0; k < C; ++k) {
        const lpf_outputs &o = out[k];
        const LpfParams &P = A.P[k];
        if (o.on_device) continue;
        any_host = true;
        const int nMB = P.M * c->cams.bx[k].total();
        if ((rc = narrow_back_a(c, o, P, n, nMB, hs.data() + (size_t)k * F, &later[k]))) return rc;
        lists_later |= later[k];
    }
    if (lists_later) {
        LPF_HIP(c, host_wait(c));
        for (int k = 0; k < C; ++k)
            if (later[k] && (rc = narrow_back_b(c, out[k], A.P[k], frame_off, hs.data() + (size_t)k * F))) return rc;
    }
    if (any_host || host_in) LPF_HIP(c, host_wait(c));         // host buffers are filled, or may be reused
    return LPF_OK;
}

// ---- lpf_run_cams_wide (include/lpf.h): one scan in up to LPF_MAX_CAMS cameras of up to LPF_MAX_MASKS_WIDE masks each, kernels in
// lpf_cams_wide.hip.h.  Camera c runs lpf_run_wide's chain on buffers of its own (c->camsw.cam[c]) with lpf_run_cams' box tables
// (c->cams.bx[c]); one projecting launch reads the points once for every camera, and each later stage is one launch for all of them.
int lpf_run_cams_wide(lpf_ctx *c, const float *pts, const int64_t *frame_off, int F, int pts_on_device, const lpf_cam_input *cams, int C,
                      const lpf_wide_outputs *out)
{
    int rc;
    if ((rc = cams_check(c, "lpf_run_cams_wide", pts, frame_off, F, cams, C, out, LPF_WIDE_CHUNK, LPF_MAX_MASKS_WIDE,
                         "a pass takes 0 .. LPF_MAX_MASKS_WIDE", " per camera")))
        return rc;
    for (int k = 0; k < C; ++k)
        if (out[k].inst_idx && out[k].inst_cap <= 0)
            return fail(c, LPF_ERR_ARG, "run_cams_wide: out[%d].inst_idx given with inst_cap=%lld", k, (long long)out[k].inst_cap);
    // a software-pipelined context launches what it owes first (no host wait): everything below runs in stream order behind it
    if ((rc = flush_pending(c))) return rc;
    const size_t n = (size_t)frame_off[F];
    bool host_in = false;

    // ---- points: read once by the projecting launch ---------------------------------------------------------------------------------
    const float4 *d_pts;
    if ((rc = host_points(c, c->camsw.pts, pts, pts_on_device != 0, 0, n, n, &d_pts, &host_in))) return rc;

    // ---- frame tables, one per camera (the chunk fields depend on the points only, the box fields on the camera's boxes) -----------
    std::vector<LpfWideFrame> fr((size_t)C * F);
    int nchunk = 0, Btot[LPF_MAX_CAMS] = {0, 0, 0, 0}, nbw[LPF_MAX_CAMS] = {0, 0, 0, 0};
    for (int k = 0; k < C; ++k) {
        if ((rc = cams_box_tables(c, cams[k], k, F))) return rc;
        const lpf_ctx::BoxSet &BX = c->cams.bx[k];
        Btot[k] = BX.total();
        nchunk = wide_frames(frame_off, F, BX, fr.data() + (size_t)k * F, &nbw[k]);
    }
    if ((rc = reserve(c, c->camsw.tab, fr.size() * sizeof(LpfWideFrame)))) return rc;
    if ((rc = upload(c, c->camsw.tab.p, fr.data(), fr.size() * sizeof(LpfWideFrame)))) return rc;

    // ---- per camera: its lpf_run_wide parameters, masks -> planes, outputs and scratch ---------------------------------------------
    LpfCamsWideArgs A;
    memset(&A, 0, sizeof A);
    A.C = C;
    Stage S[LPF_MAX_CAMS];
    int max_lists = 0, max_boxes = 0;
    bool any_boxes = false, any_host = false;
    for (int k = 0; k < C; ++k) {
        const lpf_cam_input &I = cams[k];
        const lpf_ctx::BoxSet &BX = c->cams.bx[k];
        lpf_ctx::Wide &D = c->camsw.cam[k];
        LpfWideParams &W = A.P[k];
        const int M = I.masks.M, LW = (M + 31) / 32;
        wide_params(W, input_cam(I), F, M, nchunk, nbw[k], BX, out[k].inst_cap, (const LpfWideFrame *)c->camsw.tab.p + (size_t)k * F);
        W.pts = d_pts;
        if ((rc = wide_pack(c, D, PlaneSource(I.masks, c->rle_in[k]), F, I.W, I.H, &W.planes, &host_in))) return rc;
        if ((rc = wide_bind(c, D, &out[k], n, F, Btot[k], W, S[k]))) return rc;
        max_lists = std::max(max_lists, F * std::max(LW, 1));
        if (M > 0 && Btot[k] > 0) {
            any_boxes = true;
            max_boxes = std::max(max_boxes, F * LW * nbw[k]);
        }
        any_host |= !out[k].on_device;
    }

    // ---- the launch set: each stage once for every camera --------------------------------------------------------------------------
    if (nchunk > 0) {
        hipLaunchKernelGGL(lpf_cams_wide_project, dim3((unsigned)nchunk), dim3(LPF_BLOCK), 0, c->stream, A);
        LPF_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(lpf_cams_wide_scan, dim3((unsigned)F, (unsigned)C), dim3(LPF_BLOCK), 0, c->stream, A);
    LPF_HIP(c, hipGetLastError());
    if (nchunk > 0) {
        hipLaunchKernelGGL(lpf_cams_wide_scatter, dim3((unsigned)nchunk, (unsigned)C), dim3(LPF_BLOCK), 0, c->stream, A);
        LPF_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(lpf_cams_wide_lists, dim3((unsigned)max_lists, (unsigned)C), dim3(LPF_BLOCK), 0, c->stream, A);
    LPF_HIP(c, hipGetLastError());
    if (any_boxes) {
        for (int k = 0; k < C; ++k)
            if (A.P[k].M > 0 && Btot[k] > 0) LPF_HIP(c, hipMemsetAsync(A.P[k].cnt, 0, (size_t)A.P[k].M * Btot[k] * 4, c->stream));
        hipLaunchKernelGGL(lpf_cams_wide_boxes, dim3((unsigned)max_boxes, LPF_WIDE_PARTS, (unsigned)C), dim3(LPF_BLOCK), 0, c->stream, A);
        LPF_HIP(c, hipGetLastError());
    }
    bool any_masks = false;
    for (int k = 0; k < C; ++k) any_masks |= A.P[k].M > 0;
    if (any_masks) {
        hipLaunchKernelGGL(lpf_cams_wide_best, dim3((unsigned)F, (unsigned)C), dim3(LPF_BLOCK), 0, c->stream, A);
        LPF_HIP(c, hipGetLastError());
    }

    for (int k = 0; k < C; ++k)
        if (!out[k].on_device && (rc = S[k].back(c))) return rc;
    if (any_host || host_in) LPF_HIP(c, host_wait(c));       // host buffers are filled, or may be reused
    return LPF_OK;
}

int lpf_run(lpf_ctx *c, const float *pts, int64_t N, int pts_on_device, const lpf_outputs *out)
{
    const int64_t off[2] = {0, N};
    return lpf_run_batch(c, pts, off, 1, pts_on_device, out);
}

// one frame of a stream in one call: masks (+ rectangles), boxes, run (include/lpf.h)
int lpf_run_frame(lpf_ctx *c, const lpf_frame_job *j)
{
    if (!c) return LPF_ERR_ARG;
    if (!j) return fail(c, LPF_ERR_ARG, "lpf_run_frame: job is NULL");
    if (!j->out.on_device) return fail(c, LPF_ERR_ARG, "lpf_run_frame: device-mode outputs only (out.on_device = 1)");
    if (j->n_masks < 0 || j->n_boxes < 0) return fail(c, LPF_ERR_ARG, "lpf_run_frame: n_masks=%d n_boxes=%d", j->n_masks, j->n_boxes);
    int rc;
    if (j->masks) {
        if (j->mask_rects && (rc = lpf_set_mask_rects(c, j->mask_rects, 1, 1, j->n_masks))) return rc;
        if ((rc = lpf_set_masks_u8(c, j->masks, 1, j->n_masks, 0, 2))) return rc;
    }
    if (j->corners_cam0) {
        const int32_t boff[2] = {0, j->n_boxes};
        if ((rc = lpf_set_boxes_cam0(c, j->corners_cam0, 2, boff, 1, j->T_cam_to_velo, j->filter_visible, j->oriented, nullptr, nullptr, nullptr, nullptr)))
            return rc;
    }
    return lpf_run(c, j->pts, j->n_points, 1, &j->out);
}

// one frame of a stream with up to LPF_MAX_MASKS_WIDE masks in one call: boxes, then lpf_run_wide's run (include/lpf.h).  A sparse
// frame (lpf_run_batch's sparse_frames rule) with rectangles and at most LPF_FW_DIRECT_MAX masks reads its masks directly
// (lpf_wide_direct_project): M reads per valid point, gated by the rectangles, against M reads per pixel for the pack.  Measured on
// the four full-size golden frames: 36.2 against 46.2 us at 40 masks, 68.4 against 66.6 at 64, and further
// behind at 128 and 256 -- a real frame's ~115 chunks are too few blocks to hide a candidate walk that long, while the pack spreads
// over the whole image.
#define LPF_FW_DIRECT_MAX 48
int lpf_run_frame_wide(lpf_ctx *c, const lpf_frame_job_wide *j)
{
    if (!c) return LPF_ERR_ARG;
    if (!j) return fail(c, LPF_ERR_ARG, "lpf_run_frame_wide: job is NULL");
    if (c->capturing) return fail(c, LPF_ERR_STATE, "lpf_run_frame_wide cannot be captured into a graph (call it outside lpf_graph_begin ... lpf_graph_end)");
    if (j->out.on_device != 1) return fail(c, LPF_ERR_ARG, "lpf_run_frame_wide: device-mode outputs only (out.on_device = 1)");
    if (j->n_masks < 0 || j->n_masks > LPF_MAX_MASKS_WIDE || j->n_boxes < 0)
        return fail(c, LPF_ERR_ARG, "lpf_run_frame_wide: n_masks=%d (0 .. LPF_MAX_MASKS_WIDE = %d) n_boxes=%d", j->n_masks, LPF_MAX_MASKS_WIDE,
                    j->n_boxes);
    if (j->n_masks > 0 && !j->masks) return fail(c, LPF_ERR_ARG, "lpf_run_frame_wide: masks is NULL with n_masks=%d", j->n_masks);
    if (!c->have_camera) return fail(c, LPF_ERR_STATE, "lpf_set_camera has not been called");
    int rc;
    if (j->corners_cam0) {
        const int32_t boff[2] = {0, j->n_boxes};
        if ((rc = lpf_set_boxes_cam0(c, j->corners_cam0, 2, boff, 1, j->T_cam_to_velo, j->filter_visible, j->oriented, nullptr, nullptr, nullptr, nullptr)))
            return rc;
    }
    lpf_wide_input in;
    memset(&in, 0, sizeof in);
    in.masks = j->masks;
    in.rects = j->mask_rects;
    in.M = j->n_masks;
    in.on_device = 2;
    const int64_t off[2] = {0, j->n_points};
    const bool direct = j->mask_rects && ((uintptr_t)j->mask_rects & 15) == 0 && j->n_masks > 0 && j->n_masks <= LPF_FW_DIRECT_MAX &&
                        2 * j->n_points <= (int64_t)c->W * c->H;
    return run_wide_input(c, j->pts, off, 1, 1, &in, &j->out, direct);
}

}  // extern "C"

#include "lpf_reader.hip.h"
