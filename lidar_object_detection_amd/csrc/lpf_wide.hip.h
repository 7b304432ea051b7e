// lpf_wide.hip.h -- frames with up to LPF_MAX_MASKS_WIDE (256) masks in one pass (lpf_run_wide, include/lpf.h).
//
// A point's membership is LW = ceil(M / 32) label words instead of one.  Everything per point is the narrow path's own device code
// -- the k-ordered f64 transform and the clip (lpf_project_point, lpf_pixel), the membership rules (lpf_member), the erosion
// (the plus-shaped AND of lpf_pack_erode, and lpf_erode_packed itself for the further iterations), the box tests (boxq bounds, then
// lpf_oriented_inside / lpf_aabb_inside) and the first strict maximum of lpf_finalize_frame -- so a wide run is bit-equal to the
// narrow one run once per group of 32 masks.  The kernels here are separate launches in stream order: nothing waits for another
// block.
//   lpf_wide_pack     masks [F][M][H][W] -> LW planes [F][LW][H][W] of u32 (+ the first erosion, LDS tile as lpf_pack_erode)
//   lpf_wide_project  1024-point chunks: uv / depth / u_f / v_f, the LW words of a valid point, per-chunk valid / masked counts
//   lpf_wide_scan     one block per frame: chunk prefixes, n_valid, n_labelled
//   lpf_wide_scatter  valid_idx, uv_valid, label_valid_words, and the frame's masked valid points (index, words, xyz) in point order
//   lpf_wide_lists    one block per (frame, label word): instance counts, offsets and lists of its 32 masks from the masked list
//   lpf_wide_boxes    per (frame, label word, 64-box word, part of the masked list): inside counts into [M][B]
//   lpf_wide_best     one block per frame: count_mb and the first strict maximum per mask
#pragma once
#include "lpf_kernels.hip.h"

#define LPF_MAX_MASKS_WIDE_DEV 256     // = LPF_MAX_MASKS_WIDE of include/lpf.h
#define LPF_WIDE_CHUNK 1024            // points per lpf_wide_project / lpf_wide_scatter block: 4 consecutive points per thread
#define LPF_WIDE_PARTS 8               // parts of a frame's masked list per box-count block

struct LpfWideFrame {                  // per frame (host-built, uploaded)
    long long pt_off;                  // first point in the concatenated arrays
    int N;                             // points
    int chunk_off;                     // first chunk
    int nchunk;
    int box_off, B;                    // boxes of the frame
    int pad;
};

struct LpfWideParams {
    LpfCam cam;
    int F, M, LW, nchunk, nbw;         // nbw: 64-box words of the frame with the most boxes
    int oriented;
    long long inst_cap;
    const LpfWideFrame *frames;        // [F]
    const float4 *pts;
    const uint32_t *planes;            // [F][LW][H][W]
    const double *boxp;                // [Btot][16]
    const float *boxq;                 // [Btot][8]
    // outputs (nullable unless noted)
    int2 *uv;                          // never null (uv_valid is gathered from it)
    double *depth, *uf, *vf;
    long long *valid_idx;
    int2 *uv_valid;
    uint32_t *label_words;             // [Ntot][LW], never null
    uint32_t *label_valid;             // [Ntot][LW]
    long long *inst_idx;
    int32_t *count_out;                // [M * Btot]
    long long *n_valid, *n_labelled, *inst_count, *inst_off, *best_cnt;
    int32_t *best_box, *inst_overflow;
    // scratch
    uint32_t *flags;                   // [nchunk][LPF_WIDE_CHUNK / 4] bytes of 4 points: bit 0 valid, bit 1 masked
    int2 *chunk_cnt, *chunk_pre;       // [nchunk] {valid, masked}
    int2 *fcnt;                        // [F] {n_valid, n_masked}
    int *m_idx;                        // [Ntot] frame f's masked valid points (frame-relative index) at pt_off, in point order
    uint32_t *m_words;                 // [Ntot][LW] their words
    float4 *m_pts;                     // [Ntot] their xyz
    unsigned *cnt;                     // [M * Btot] inside counts (zeroed before the launch set)
};

__device__ __forceinline__ int lpf_wide_frame_of_chunk(const LpfWideParams &W, const int c)
{
    int lo = 0, hi = W.F - 1;                                // last frame whose chunk_off <= c (frames of no chunk are skipped)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (W.frames[mid].chunk_off <= c) lo = mid; else hi = mid - 1;
    }
    while (W.frames[lo].nchunk == 0 && lo > 0) --lo;
    return lo;
}

// exclusive prefix over the 256 threads of a block and the block total (s: 4 words of LDS)
__device__ __forceinline__ unsigned lpf_wide_block_excl(unsigned v, unsigned *s, unsigned &total)
{
    const int lane = lpf_lane(), wave = lpf_wave();
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(incl, o);
        if (lane >= o) incl += t;
    }
    __syncthreads();
    if (lane == 63) s[wave] = incl;
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += s[w];
    total = s[0] + s[1] + s[2] + s[3];
    return before + incl - v;
}

// ---- masks -> LW label planes, first erosion fused (the lpf_pack_erode tile: pixels outside the image read as all ones) ----------
template <typename T, int MODE>
__global__ __launch_bounds__(LPF_BLOCK) void lpf_wide_pack(const T *__restrict__ masks, uint32_t *__restrict__ planes, int M, int LW,
                                                           int H, int W, int erode, const int4 *__restrict__ rects)
{
    __shared__ uint32_t s_tile[LPF_TH + 2][LPF_TW + 2 + 1];
    const int f = blockIdx.z / LW, wd = blockIdx.z - f * LW;
    const int m0 = 32 * wd, mw = min(32, M - m0);
    const int x0 = blockIdx.x * LPF_TW, y0 = blockIdx.y * LPF_TH;
    const size_t hw = (size_t)H * W;
    const T *__restrict__ mf = masks + ((size_t)f * M + m0) * hw;
    const int4 *__restrict__ rf = rects ? rects + (size_t)f * M + m0 : nullptr;
    // the word's masks whose rectangle meets this tile (halo included): the others are zero here and not read
    unsigned live = mw >= 32 ? 0xFFFFFFFFu : ((1u << mw) - 1u);
    if (rf) {
        for (int j = 0; j < mw; ++j) {
            const int4 r = rf[j];
            if (r.z <= x0 - 1 || r.x >= x0 + LPF_TW + 1 || r.w <= y0 - 1 || r.y >= y0 + LPF_TH + 1 || r.z <= r.x || r.w <= r.y) live &= ~(1u << j);
        }
    }
    for (int p = threadIdx.x; p < (LPF_TH + 2) * (LPF_TW + 2); p += LPF_BLOCK) {
        const int ty = p / (LPF_TW + 2), tx = p - ty * (LPF_TW + 2);
        const int y = y0 + ty - 1, x = x0 + tx - 1;
        uint32_t bits = 0xFFFFFFFFu;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            bits = 0;
            const size_t o = (size_t)y * W + x;
            unsigned rest = live;
            while (rest) {
                const int j = __ffs(rest) - 1;
                rest &= rest - 1u;
                if (rf) {                                   // (lpf_set_mask_rects' contract: zero outside the rectangle, pixel for pixel)
                    const int4 r = rf[j];
                    if (!(x >= r.x && x < r.z && y >= r.y && y < r.w)) continue;
                }
                if (lpf_member<T, MODE>(mf[(size_t)j * hw + o])) bits |= 1u << j;
            }
        }
        s_tile[ty][tx] = bits;
    }
    __syncthreads();
    const int tx = threadIdx.x & (LPF_TW - 1);
    uint32_t *__restrict__ dst = planes + ((size_t)f * LW + wd) * hw;
    for (int ty = threadIdx.x >> 6; ty < LPF_TH; ty += LPF_BLOCK / LPF_TW) {
        const int y = y0 + ty, x = x0 + tx;
        if (y < H && x < W) {
            uint32_t v = s_tile[ty + 1][tx + 1];
            if (erode) v &= s_tile[ty][tx + 1] & s_tile[ty + 2][tx + 1] & s_tile[ty + 1][tx] & s_tile[ty + 1][tx + 2];
            dst[(size_t)y * W + x] = v;
        }
    }
}

// The same with the first erosion by the k x k MORPH_ELLIPSE element of lpf_set_erosion_element, k = 5 .. 15 (lpf_pack_erode_k's tile
// and AND, a plane per (frame, word)).  No rectangles: they hold without erosion only (rects_hold).
template <typename T, int MODE>
__global__ __launch_bounds__(LPF_BLOCK) void lpf_wide_pack_k(const T *__restrict__ masks, uint32_t *__restrict__ planes, int M, int LW,
                                                             int H, int W, int r, uint32_t spans)
{
    __shared__ uint32_t s_tile[LPF_EK_ROWS][LPF_EK_LD];
    const int f = blockIdx.z / LW, wd = blockIdx.z - f * LW;
    const int m0 = 32 * wd, mw = min(32, M - m0);
    const int x0 = blockIdx.x * LPF_TW, y0 = blockIdx.y * LPF_TH;
    const size_t hw = (size_t)H * W;
    lpf_element_stage_masks<T, MODE>(s_tile, masks + ((size_t)f * M + m0) * hw, mw, hw, H, W, x0, y0, r);
    __syncthreads();
    const int tx = threadIdx.x & (LPF_TW - 1);
    uint32_t *__restrict__ dst = planes + ((size_t)f * LW + wd) * hw;
    for (int ty = threadIdx.x >> 6; ty < LPF_TH; ty += LPF_BLOCK / LPF_TW) {
        const int y = y0 + ty, x = x0 + tx;
        if (y < H && x < W) dst[(size_t)y * W + x] = lpf_element_and(s_tile, ty, tx, r, spans);
    }
}

// ---- project + label: 1024 points per block, 4 consecutive points per thread ----------------------------------------------------
// The two ends of a chunk, shared by its packed (lpf_wide_project_chunk) and direct (lpf_wide_direct_project) forms.
// Point p at g of the concatenated arrays: uv / depth / u_f / v_f, its pixel, and whether it is valid.
__device__ __forceinline__ bool lpf_wide_project_point(const LpfWideParams &W, const size_t g, const float4 p, int &ui, int &vi)
{
    double uf, vf, d;
    lpf_project_point(W.cam, p.x, p.y, p.z, uf, vf, d);
    const bool ok = lpf_pixel(W.cam, uf, vf, d, ui, vi);
    W.uv[g] = make_int2(ui, vi);
    if (W.depth) W.depth[g] = d;
    if (W.uf) W.uf[g] = uf;
    if (W.vf) W.vf[g] = vf;
    return ok;
}

// The thread's flags word (a byte per point: bit 0 valid, bit 1 masked) and chunk c's counts of both (s_tmp: 8 words of LDS).
__device__ __forceinline__ void lpf_wide_chunk_end(const LpfWideParams &W, const int c, const unsigned fl, unsigned *s_tmp)
{
    W.flags[(size_t)c * (LPF_WIDE_CHUNK / 4) + threadIdx.x] = fl;
    unsigned tv, tm;
    lpf_wide_block_excl(__popc(fl & 0x01010101u), s_tmp, tv);
    lpf_wide_block_excl(__popc(fl & 0x02020202u), s_tmp + 4, tm);
    if (threadIdx.x == 0) W.chunk_cnt[c] = make_int2((int)tv, (int)tm);
}

// Chunk c of frame f (chunk_off and the points depend on the points only: every camera of lpf_cams_wide_project finds the same ones).
// PRE: the thread's four points are in p[] already (lpf_cams_wide_project loads them once for every camera); else each is read here.
template <bool PRE>
__device__ __forceinline__ void lpf_wide_project_chunk(const LpfWideParams &W, const int c, const int f, const LpfWideFrame &fr,
                                                       const float4 *p_pre, unsigned *s_tmp)
{
    const int base = (c - fr.chunk_off) * LPF_WIDE_CHUNK;
    const size_t hw = (size_t)W.cam.W * (size_t)W.cam.H;
    const uint32_t *__restrict__ pl = W.planes ? W.planes + (size_t)f * W.LW * hw : nullptr;
    unsigned fl = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = base + threadIdx.x * 4 + r;          // frame-relative point
        if (i >= fr.N) break;
        const size_t g = (size_t)fr.pt_off + i;
        int ui, vi;
        const bool ok = lpf_wide_project_point(W, g, PRE ? p_pre[r] : W.pts[g], ui, vi);
        unsigned any = 0;
        uint32_t *__restrict__ lw = W.label_words + g * W.LW;
        if (ok && pl) {
            const size_t pix = (size_t)vi * W.cam.W + ui;
            for (int w = 0; w < W.LW; ++w) { const uint32_t v = pl[(size_t)w * hw + pix]; lw[w] = v; any |= v; }
        } else {
            for (int w = 0; w < W.LW; ++w) lw[w] = 0u;
        }
        fl |= ((ok ? 1u : 0u) | (any ? 2u : 0u)) << (8 * r);
    }
    lpf_wide_chunk_end(W, c, fl, s_tmp);
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_wide_project(const LpfWideParams W)
{
    __shared__ unsigned s_tmp[8];
    const int c = blockIdx.x;
    const int f = lpf_wide_frame_of_chunk(W, c);
    const LpfWideFrame fr = W.frames[f];
    lpf_wide_project_chunk<false>(W, c, f, fr, nullptr, s_tmp);
}

// ---- per frame: chunk prefixes and the frame's totals -------------------------------------------------------------------------
__device__ __forceinline__ void lpf_wide_scan_frame(const LpfWideParams &W, const int f, unsigned *s_tmp)
{
    const LpfWideFrame fr = W.frames[f];
    unsigned cv = 0, cm = 0;
    for (int k0 = 0; k0 < fr.nchunk; k0 += LPF_BLOCK) {
        const int k = k0 + threadIdx.x;
        const int2 v = k < fr.nchunk ? W.chunk_cnt[fr.chunk_off + k] : make_int2(0, 0);
        unsigned tv, tm;
        const unsigned ev = lpf_wide_block_excl((unsigned)v.x, s_tmp, tv);
        const unsigned em = lpf_wide_block_excl((unsigned)v.y, s_tmp + 4, tm);
        if (k < fr.nchunk) W.chunk_pre[fr.chunk_off + k] = make_int2((int)(cv + ev), (int)(cm + em));
        cv += tv; cm += tm;
    }
    if (threadIdx.x == 0) {
        W.fcnt[f] = make_int2((int)cv, (int)cm);
        if (W.n_valid) W.n_valid[f] = cv;
        if (W.n_labelled) W.n_labelled[f] = cm;
    }
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_wide_scan(const LpfWideParams W)
{
    __shared__ unsigned s_tmp[8];
    lpf_wide_scan_frame(W, blockIdx.x, s_tmp);
}

// ---- compact outputs and the masked list ---------------------------------------------------------------------------------------
__device__ __forceinline__ void lpf_wide_scatter_chunk(const LpfWideParams &W, const int c, unsigned *s_tmp)
{
    const int f = lpf_wide_frame_of_chunk(W, c);
    const LpfWideFrame fr = W.frames[f];
    const int base = (c - fr.chunk_off) * LPF_WIDE_CHUNK;
    const unsigned fl = W.flags[(size_t)c * (LPF_WIDE_CHUNK / 4) + threadIdx.x];
    unsigned nv = 0, nm = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) { nv += (fl >> (8 * r)) & 1u; nm += (fl >> (8 * r + 1)) & 1u; }
    unsigned tv, tm;
    const int2 pre = W.chunk_pre[c];
    unsigned pv = (unsigned)pre.x + lpf_wide_block_excl(nv, s_tmp, tv);
    unsigned pm = (unsigned)pre.y + lpf_wide_block_excl(nm, s_tmp + 4, tm);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned b = (fl >> (8 * r)) & 3u;
        if (!b) continue;
        const int i = base + threadIdx.x * 4 + r;
        const size_t g = (size_t)fr.pt_off + i;
        const size_t gv = (size_t)fr.pt_off + pv;
        if (W.valid_idx) W.valid_idx[gv] = i;
        if (W.uv_valid) W.uv_valid[gv] = W.uv[g];
        if (W.label_valid) for (int w = 0; w < W.LW; ++w) W.label_valid[gv * W.LW + w] = W.label_words[g * W.LW + w];
        ++pv;
        if (b & 2u) {
            const size_t gm = (size_t)fr.pt_off + pm;
            W.m_idx[gm] = i;
            for (int w = 0; w < W.LW; ++w) W.m_words[gm * W.LW + w] = W.label_words[g * W.LW + w];
            const float4 p = W.pts[g];
            W.m_pts[gm] = make_float4(p.x, p.y, p.z, 0.f);
            ++pm;
        }
    }
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_wide_scatter(const LpfWideParams W)
{
    __shared__ unsigned s_tmp[8];
    lpf_wide_scatter_chunk(W, blockIdx.x, s_tmp);
}

// ---- instance counts, offsets and lists: block (frame, word) ---------------------------------------------------------------------
// Offsets need the counts of every earlier mask of the frame: the block sums the popcounts of the earlier words of each masked entry
// itself (a few thousand entries), so no block waits for another.
// (blk: frame * max(LW, 1) + word; LDS: s_cnt[32], s_run[32], s_wc[4][32], s_before)
__device__ __forceinline__ void lpf_wide_lists_block(const LpfWideParams &W, const int blk, unsigned *s_cnt, unsigned *s_run,
                                                     unsigned (*s_wc)[32], unsigned &s_before)
{
    const int f = blk / max(W.LW, 1), wd = blk - f * max(W.LW, 1);
    const int lane = lpf_lane(), wave = lpf_wave(), tid = threadIdx.x;
    const LpfWideFrame fr = W.frames[f];
    const int n = W.fcnt[f].y;
    const int mw = min(32, W.M - 32 * wd);
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (tid < 32) s_cnt[tid] = 0u;
    if (tid == 0) s_before = 0u;
    __syncthreads();
    unsigned acc = 0, before = 0;
    for (int e0 = 0; e0 < n; e0 += LPF_BLOCK) {
        const int e = e0 + tid;
        uint32_t x = 0;
        if (e < n) {
            const uint32_t *__restrict__ mw_ = W.m_words + ((size_t)fr.pt_off + e) * W.LW;
            x = mw_[wd];
            for (int w = 0; w < wd; ++w) before += __popc(mw_[w]);
        }
        for (int b = 0; b < 32; ++b) {
            const unsigned k = (unsigned)__popcll(__ballot((x >> b) & 1u));
            if (lane == b) acc += k;
        }
    }
    if (lane < 32 && acc) atomicAdd(&s_cnt[lane], acc);
    if (before) atomicAdd(&s_before, before);
    __syncthreads();
    if (wave == 0) {                                        // offsets of the word's masks
        const unsigned c = lane < mw ? s_cnt[lane] : 0u;
        unsigned incl = c;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const unsigned t = __shfl_up(incl, o);
            if (lane >= o) incl += t;
        }
        const long long off = (long long)s_before + incl - c;
        if (lane < mw) {
            const int m = 32 * wd + lane;
            if (W.inst_count) W.inst_count[(size_t)f * W.M + m] = c;
            if (W.inst_off) W.inst_off[(size_t)f * (W.M + 1) + m] = off;
            s_run[lane] = (unsigned)off;
            if (lane == mw - 1 && 32 * wd + mw == W.M) {    // the frame's last mask: total, overflow
                if (W.inst_off) W.inst_off[(size_t)f * (W.M + 1) + W.M] = off + c;
                if (W.inst_overflow) W.inst_overflow[f] = (W.inst_idx && off + c > W.inst_cap) ? 1 : 0;
            }
        }
        if (W.M == 0 && lane == 0) {                        // (no masks: one block per frame writes the empty summary)
            if (W.inst_off) W.inst_off[(size_t)f] = 0;
            if (W.inst_overflow) W.inst_overflow[f] = 0;
        }
    }
    if (!W.inst_idx || mw <= 0) return;
    __syncthreads();
    long long *__restrict__ dst = W.inst_idx + (size_t)f * W.inst_cap;
    for (int e0 = 0; e0 < n; e0 += LPF_BLOCK) {             // stable: entries in point order, waves in order, lanes in order
        const int e = e0 + tid;
        const uint32_t x = e < n ? W.m_words[((size_t)fr.pt_off + e) * W.LW + wd] : 0u;
        for (int b = 0; b < mw; ++b) {
            const unsigned long long bal = __ballot((x >> b) & 1u);
            if (lane == 0) s_wc[wave][b] = (unsigned)__popcll(bal);
        }
        __syncthreads();
        if (x) {
            const int idx = W.m_idx[(size_t)fr.pt_off + e];
            for (int b = 0; b < mw; ++b) {
                const unsigned long long bal = __ballot((x >> b) & 1u);      // (active lanes only: the bits of the others are zero anyway)
                if ((x >> b) & 1u) {
                    unsigned pos = s_run[b] + (unsigned)__popcll(bal & lt);
                    for (int w = 0; w < wave; ++w) pos += s_wc[w][b];
                    if ((long long)pos < W.inst_cap) dst[pos] = idx;
                }
            }
        }
        __syncthreads();
        if (tid < mw) s_run[tid] += s_wc[0][tid] + s_wc[1][tid] + s_wc[2][tid] + s_wc[3][tid];
        __syncthreads();
    }
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_wide_lists(const LpfWideParams W)
{
    __shared__ unsigned s_cnt[32], s_run[32], s_wc[4][32], s_before;
    lpf_wide_lists_block(W, blockIdx.x, s_cnt, s_run, s_wc, s_before);
}

// ---- box counts: block (frame, word, 64-box word, part); a lane per masked entry, the boxes from LDS ----------------------------
// (blk: (frame * LW + word) * nbw + 64-box word; LDS: s_bp[64 * 16], s_bq[64 * 6], s_c[32 * 64])
__device__ __forceinline__ void lpf_wide_boxes_block(const LpfWideParams &W, const int blk, const int part, double *s_bp, float *s_bq,
                                                     unsigned *s_c)
{
    const int per_f = W.LW * W.nbw;
    const int f = blk / per_f, rem = blk - f * per_f;
    const int wd = rem / W.nbw, bw = rem - wd * W.nbw;
    const int tid = threadIdx.x;
    const LpfWideFrame fr = W.frames[f];
    const int b0 = 64 * bw, nb = min(64, fr.B - b0);
    if (nb <= 0) return;
    const int n = W.fcnt[f].y;
    const int lo = (int)((long long)n * part / LPF_WIDE_PARTS), hi = (int)((long long)n * (part + 1) / LPF_WIDE_PARTS);
    if (lo >= hi) return;
    const double *__restrict__ bp = W.boxp + ((size_t)fr.box_off + b0) * 16;
    const float *__restrict__ bq = W.boxq + ((size_t)fr.box_off + b0) * 8;     // {lo xyz, -, hi xyz, -}
    for (int i = tid; i < nb * 16; i += LPF_BLOCK) s_bp[i] = bp[i];
    for (int i = tid; i < nb * 6; i += LPF_BLOCK) { const int bx = i / 6, j = i - 6 * bx; s_bq[i] = bq[8 * bx + (j < 3 ? j : j + 1)]; }
    for (int i = tid; i < 32 * 64; i += LPF_BLOCK) s_c[i] = 0u;
    __syncthreads();
    for (int e = lo + tid; e < hi; e += LPF_BLOCK) {
        const size_t ge = (size_t)fr.pt_off + e;
        const uint32_t x = W.m_words[ge * W.LW + wd];
        if (!x) continue;
        const float4 p = W.m_pts[ge];
        const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
        for (int j = 0; j < nb; ++j) {
            const float *q = s_bq + 6 * j;
            if (!(p.x >= q[0] && p.x <= q[3] && p.y >= q[1] && p.y <= q[4] && p.z >= q[2] && p.z <= q[5])) continue;
            const bool in = W.oriented ? lpf_oriented_inside(px, py, pz, s_bp + 16 * j) : lpf_aabb_inside(px, py, pz, s_bp + 16 * j);
            if (!in) continue;
            uint32_t l = x;
            while (l) {
                const int b = __ffs(l) - 1;
                l &= l - 1u;
                atomicAdd(&s_c[b * 64 + j], 1u);
            }
        }
    }
    __syncthreads();
    const int mw = min(32, W.M - 32 * wd);
    unsigned *__restrict__ cnt = W.cnt + (size_t)W.M * fr.box_off;
    for (int i = tid; i < 32 * 64; i += LPF_BLOCK) {
        const int b = i >> 6, j = i & 63;
        const unsigned v = s_c[i];
        if (v && b < mw && j < nb) atomicAdd(&cnt[(size_t)(32 * wd + b) * fr.B + b0 + j], v);
    }
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_wide_boxes(const LpfWideParams W)
{
    __shared__ double s_bp[64 * 16];
    __shared__ float s_bq[64 * 6];
    __shared__ unsigned s_c[32 * 64];
    lpf_wide_boxes_block(W, blockIdx.x, blockIdx.y, s_bp, s_bq, s_c);
}

// ---- per frame: count_mb and the first strict maximum per mask (lpf_finalize_frame's rule) --------------------------------------
__device__ __forceinline__ void lpf_wide_best_frame(const LpfWideParams &W, const int f)
{
    const int lane = lpf_lane(), wave = lpf_wave();
    const LpfWideFrame fr = W.frames[f];
    const int B = fr.B, M = W.M;
    const unsigned *__restrict__ cnt = W.cnt + (size_t)M * fr.box_off;
    if (W.count_out)
        for (int i = threadIdx.x; i < M * B; i += LPF_BLOCK) W.count_out[(size_t)M * fr.box_off + i] = (int32_t)cnt[i];
    for (int m = wave; m < M; m += 4) {
        unsigned best = 0;
        int best_idx = 0x7fffffff;
        for (int b = lane; b < B; b += 64) {
            const unsigned c = cnt[(size_t)m * B + b];
            if (c > best) { best = c; best_idx = b; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned ob = __shfl_down(best, o);
            const int oi = __shfl_down(best_idx, o);
            if (ob > best || (ob == best && oi < best_idx)) { best = ob; best_idx = oi; }
        }
        if (lane == 0) {
            if (W.best_cnt) W.best_cnt[(size_t)f * M + m] = (long long)best;
            if (W.best_box) W.best_box[(size_t)f * M + m] = best ? best_idx : -1;
        }
    }
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_wide_best(const LpfWideParams W) { lpf_wide_best_frame(W, blockIdx.x); }
