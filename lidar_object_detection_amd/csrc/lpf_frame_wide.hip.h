// lpf_frame_wide.hip.h -- the projecting stage of lpf_run_frame_wide (include/lpf.h) for sparse frames with mask rectangles: the lent
// uint8 masks are read where a valid point falls, inside the mask's rectangle, instead of being packed into ceil(M / 32) full-image
// u32 planes first (lpf_wide_pack: M reads per pixel of the image against M reads per valid point here, gated by the rectangles).
//
//   lpf_wide_direct_project  one LPF_WIDE_CHUNK chunk per block, 4 consecutive points per thread, as lpf_wide_project; it writes what
//                            lpf_wide_project writes (uv / depth / u_f / v_f, the LW label words of every point, the flags bytes,
//                            chunk_cnt), so lpf_wide_scan / _scatter / _lists / _boxes / _best run on its output unchanged.
//
// Both ends of the chunk are lpf_wide_project_chunk's own code: lpf_wide_project_point (projection, validity, the per-point stores)
// and lpf_wide_chunk_end (flags, chunk_cnt).  Only the label words between them are found differently.  Mask m contributes bit m & 31 of word m >> 5 of a valid point at (u, v) iff
//   u >= x0 && u < x1 && v >= y0 && v < y1  and  lpf_member<uint8_t, 0>(masks[m][v][u])
// -- the per-pixel test of lpf_wide_pack with rectangles, so the two forms agree even where a mask has bytes outside its rectangle.
// The rectangles are only compared, never computed with (INT32_MIN / INT32_MAX mean "no limit").
//
// A block first reduces its valid pixels to a bounding box (LDS), thread t then tests rectangle t against it (M <= 256: one rectangle
// per thread), and the masks whose rectangle meets the box are compacted, in mask order, into an LDS candidate list with the start of
// each label word's run.  Each thread walks only the candidates, word by word (the word accumulators stay in registers: no dynamically
// indexed array), and issues the byte loads of its four points for LPF_FW_CAND candidates before it consumes any of them.  Every lane
// reads the same candidate entry: an LDS broadcast.
#pragma once
#include "lpf_wide.hip.h"

#define LPF_FW_CAND 4                  // candidates whose byte loads a thread issues before it consumes any

__global__ __launch_bounds__(LPF_BLOCK) void lpf_wide_direct_project(const LpfWideParams W, const uint8_t *__restrict__ masks,
                                                                     const int4 *__restrict__ rects)
{
    __shared__ unsigned s_tmp[8];
    __shared__ int s_bb[4][4];                              // per wave: min u, max u, min v, max v of its valid points
    __shared__ int4 s_rect[LPF_MAX_MASKS_WIDE_DEV];         // candidates' rectangles, in mask order
    __shared__ int s_cid[LPF_MAX_MASKS_WIDE_DEV];           // ... their mask ids
    __shared__ int s_wst[LPF_MAX_MASKS_WIDE_DEV / 32 + 1];  // first candidate of each label word; [LW] = number of candidates
    const int c = blockIdx.x;
    const int f = lpf_wide_frame_of_chunk(W, c);
    const LpfWideFrame fr = W.frames[f];
    const int base = (c - fr.chunk_off) * LPF_WIDE_CHUNK;
    const int M = W.M, LW = W.LW, Wimg = W.cam.W;
    const size_t hw = (size_t)Wimg * (size_t)W.cam.H;
    const uint8_t *__restrict__ mf = masks + (size_t)f * M * hw;
    const int4 *__restrict__ rf = rects + (size_t)f * M;
    const int lane = lpf_lane(), wave = lpf_wave(), tid = threadIdx.x;

    // ---- project -----------------------------------------------------------------------------------------------------------------
    int pu[4], pv[4];
    unsigned okm = 0;                                       // bit r: point r is valid
    int u0 = 0x7fffffff, u1 = -1, v0 = 0x7fffffff, v1 = -1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pu[r] = 0; pv[r] = 0;
        const int i = base + tid * 4 + r;
        if (i >= fr.N) continue;
        const size_t g = (size_t)fr.pt_off + i;
        int ui, vi;
        if (lpf_wide_project_point(W, g, W.pts[g], ui, vi)) {
            okm |= 1u << r;
            pu[r] = ui; pv[r] = vi;
            u0 = min(u0, ui); u1 = max(u1, ui); v0 = min(v0, vi); v1 = max(v1, vi);
        }
    }

    // ---- the chunk's bounding box of valid pixels ------------------------------------------------------------------------------
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        u0 = min(u0, __shfl_xor(u0, o)); u1 = max(u1, __shfl_xor(u1, o));
        v0 = min(v0, __shfl_xor(v0, o)); v1 = max(v1, __shfl_xor(v1, o));
    }
    if (lane == 0) { s_bb[wave][0] = u0; s_bb[wave][1] = u1; s_bb[wave][2] = v0; s_bb[wave][3] = v1; }
    __syncthreads();
    u0 = min(min(s_bb[0][0], s_bb[1][0]), min(s_bb[2][0], s_bb[3][0]));
    u1 = max(max(s_bb[0][1], s_bb[1][1]), max(s_bb[2][1], s_bb[3][1]));
    v0 = min(min(s_bb[0][2], s_bb[1][2]), min(s_bb[2][2], s_bb[3][2]));
    v1 = max(max(s_bb[0][3], s_bb[1][3]), max(s_bb[2][3], s_bb[3][3]));

    // ---- candidates: masks whose rectangle holds a pixel of the box (no valid point: u1 = v1 = -1, none) ------------------------
    int4 rt = make_int4(0, 0, 0, 0);
    bool cand = false;
    if (tid < M) {
        rt = rf[tid];                                       // {x0, y0, x1, y1}: some u in [u0, u1] with x0 <= u < x1, same for v
        cand = rt.x < rt.z && rt.y < rt.w && rt.x <= u1 && rt.z > u0 && rt.y <= v1 && rt.w > v0;
    }
    unsigned ncand;
    const unsigned pos = lpf_wide_block_excl(cand ? 1u : 0u, s_tmp, ncand);
    if (cand) { s_rect[pos] = rt; s_cid[pos] = tid; }
    if (tid < M && (tid & 31) == 0) s_wst[tid >> 5] = (int)pos;
    if (tid == 0) s_wst[LW] = (int)ncand;
    __syncthreads();

    // ---- label words: word by word, the word's candidates against the thread's four points -------------------------------------
    size_t pix[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pix[r] = (size_t)pv[r] * Wimg + pu[r];
    unsigned any[4] = {0u, 0u, 0u, 0u};
    for (int w = 0; w < LW; ++w) {
        const int k0 = s_wst[w], k1 = s_wst[w + 1];
        unsigned acc[4] = {0u, 0u, 0u, 0u};
        if (okm) {
            for (int k = k0; k < k1; k += LPF_FW_CAND) {    // LPF_FW_CAND candidates at a time: their loads are in flight together
                int mm[LPF_FW_CAND];
                uint8_t b[LPF_FW_CAND][4];
#pragma unroll
                for (int j = 0; j < LPF_FW_CAND; ++j) {     // the loads of the four points for each candidate first ...
                    const bool live = k + j < k1;
                    const int4 q = s_rect[live ? k + j : k];
                    mm[j] = s_cid[live ? k + j : k];
                    const uint8_t *__restrict__ mk = mf + (size_t)mm[j] * hw;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        b[j][r] = 0;
                        const bool in = live && ((okm >> r) & 1u) && pu[r] >= q.x && pu[r] < q.z && pv[r] >= q.y && pv[r] < q.w;
                        if (in) b[j][r] = mk[pix[r]];
                    }
                }
#pragma unroll
                for (int j = 0; j < LPF_FW_CAND; ++j)       // ... then their bits
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (lpf_member<uint8_t, 0>(b[j][r])) acc[r] |= 1u << (mm[j] & 31);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = base + tid * 4 + r;
            if (i < fr.N) W.label_words[((size_t)fr.pt_off + i) * LW + w] = acc[r];
            any[r] |= acc[r];
        }
    }

    // ---- flags and the chunk's counts ----------------------------------------------------------------------------------------------
    unsigned fl = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) fl |= (((okm >> r) & 1u) | (any[r] ? 2u : 0u)) << (8 * r);
    lpf_wide_chunk_end(W, c, fl, s_tmp);
}
