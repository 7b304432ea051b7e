// lpf_depth_maps.hip.h -- per-car depth maps of a batch of frames as sparse lists (lpf_depth_maps, include/lpf.h).
//
// seg_with_pointcloud.py:160-170 fills depthMap_m[v,u] = depth of the last valid point inside mask m at that pixel.  The last valid
// point of a pixel wins whatever the mask, so car m of frame f is flatnonzero(where(member_m, D_f, 0)) with D_f lpf_depth_image's
// last-writer image.  The kernels below are separate launches in stream order over a chunk of frames; no block waits for another.
//   lpf_dm_winner   one thread per point: lpf_depth_image_kernel<0>'s lpf_project_point + lpf_pixel, atomicMax(win[f][pix], i + 1)
//   lpf_dm_raster   one wave per (frame, wave tile of 1024 consecutive pixels, group of 32 masks), slot k of lane l = pixel 64 k + l
//                   of the tile (the groups' counts and slots are independent: a mask's list only depends on that mask):
//                   COUNT: members per (mask, tile) with ballot + popcount, at pixels with a winner only
//                   SCATTER: the same walk again; a member's slot is its mask's offset + its tile's offset + the popcounts of the
//                   tile's earlier slots and lanes, so each car's list is in ascending pixel order.  depth is recomputed from the
//                   winning point with lpf_project_point: the bits lpf_depth_image writes.
//   lpf_dm_scan     one wave per (frame, mask): exclusive prefix of the tile counts, and the mask's total
//   lpf_dm_frame    one block per frame: exclusive prefix of the mask totals -> car_off, need, overflow
// Membership: the lent masks read where a winner is (lpf_member, the rectangles' rows and columns as a hint where lpf_wide_pack takes
// them), or -- with erosion -- bit m & 31 of lpf_wide_pack's plane m / 32.
#pragma once
#include "lpf_kernels.hip.h"
#include "lpf_wide.hip.h"

#define LPF_DM_SLOTS 16                     // pixel slots per lane
#define LPF_DM_TILE (64 * LPF_DM_SLOTS)     // pixels per wave tile
#define LPF_DM_MGROUP 32                    // masks per lpf_dm_raster wave (blockIdx.z: the group)

struct LpfDmParams {
    LpfCam cam;
    const float4 *pts;                      // the chunk's first point
    int M, LW, f0, ntile;                   // masks per frame, label words (planes), first frame of the chunk, wave tiles per frame
    long long hwp;                          // pitch of a winner plane: ntile * LPF_DM_TILE (>= W * H, zero beyond)
    long long pt_base;                      // frame_off[f0]
    long long cap;
    const long long *foff;                  // [F + 1] the batch's frame offsets
    unsigned *win;                          // [Fc][hwp] index + 1 of the winning point, 0 = none
    unsigned *cnt, *toff, *tot;             // [Fc][M][ntile] members per tile, their exclusive prefix; [Fc][M] totals
    const void *masks;                      // [Fc][M][H][W] of T, or planes [Fc][LW][H][W] u32
    const int4 *rects;                      // [Fc][M] or null
    // outputs: frame f0 + fl at row f0 + fl
    long long *pix, *pidx;
    double *depth;
    long long *car_off, *need;
    int *overflow;
};

__global__ __launch_bounds__(LPF_BLOCK) void lpf_dm_winner(const LpfDmParams P)
{
    const int fl = blockIdx.y;
    const long long a = P.foff[P.f0 + fl], n = P.foff[P.f0 + fl + 1] - a;
    const long long i = (long long)blockIdx.x * LPF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 p = P.pts[a - P.pt_base + i];
    double uf, vf, d;
    int ui, vi;
    lpf_project_point(P.cam, p.x, p.y, p.z, uf, vf, d);
    if (lpf_pixel(P.cam, uf, vf, d, ui, vi))
        atomicMax(&P.win[(size_t)fl * P.hwp + (size_t)vi * P.cam.W + ui], (unsigned)i + 1u);
}

template <typename T, int MODE, bool PLANES, bool SCATTER>
__global__ __launch_bounds__(LPF_BLOCK) void lpf_dm_raster(const LpfDmParams P)
{
    const int fl = blockIdx.y, lane = lpf_lane();
    const int wt = blockIdx.x * 4 + lpf_wave();
    if (wt >= P.ntile) return;
    const int W = P.cam.W, M = P.M;
    const long long hw = (long long)W * P.cam.H;
    const long long base = (long long)wt * LPF_DM_TILE;
    const unsigned *__restrict__ wp = P.win + (size_t)fl * P.hwp + base;
    unsigned w[LPF_DM_SLOTS], any = 0;
#pragma unroll
    for (int k = 0; k < LPF_DM_SLOTS; ++k) {
        w[k] = wp[k * 64 + lane];
        any |= w[k];
    }
    if (!__ballot(any != 0u)) return;
    const int y_lo = (int)(base / W), y_hi = (int)(min(base + LPF_DM_TILE, hw) - 1) / W;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const size_t mrow = (size_t)fl * M;
    const size_t fo = (size_t)(P.f0 + fl);
    for (int m = LPF_DM_MGROUP * blockIdx.z, m_end = min(M, m + LPF_DM_MGROUP); m < m_end; ++m) {
        const size_t mt = (mrow + m) * P.ntile + wt;
        long long run = 0;
        if (SCATTER) {
            if (P.cnt[mt] == 0u) continue;
            run = P.car_off[fo * (M + 1) + m] + P.toff[mt];
        }
        int4 r = make_int4(0, 0, 0, 0);
        if (P.rects) {
            r = P.rects[mrow + m];
            if (r.w <= y_lo || r.y > y_hi || r.z <= r.x || r.w <= r.y) continue;
        }
        unsigned c = 0;
#pragma unroll
        for (int k = 0; k < LPF_DM_SLOTS; ++k) {
            if (!__ballot(w[k] != 0u)) continue;              // (no winner in this slot of the wave)
            const long long p = base + k * 64 + lane;
            bool mem = false;
            if (w[k]) {
                bool in = true;
                if (P.rects) {                                  // (a winner's pixel is < W * H < 2^31)
                    const int y = (int)((unsigned)p / (unsigned)W), x = (int)p - y * W;
                    in = x >= r.x && x < r.z && y >= r.y && y < r.w;
                }
                if (in) {
                    if (PLANES) mem = (((const uint32_t *)P.masks)[((size_t)fl * P.LW + (m >> 5)) * hw + p] >> (m & 31)) & 1u;
                    else mem = lpf_member<T, MODE>(((const T *)P.masks)[(mrow + m) * hw + p]);
                }
            }
            const unsigned long long bal = __ballot(mem);
            if (SCATTER) {
                const long long pos = run + __popcll(bal & lt);
                if (mem && pos < P.cap) {
                    const size_t o = fo * P.cap + pos;
                    const int i = (int)(w[k] - 1u);
                    P.pix[o] = p;
                    if (P.pidx) P.pidx[o] = i;
                    if (P.depth) {
                        const float4 q = P.pts[P.foff[fo] - P.pt_base + i];
                        double uf, vf, d;
                        lpf_project_point(P.cam, q.x, q.y, q.z, uf, vf, d);
                        P.depth[o] = d;
                    }
                }
                run += __popcll(bal);
            } else {
                c += (unsigned)__popcll(bal);
            }
        }
        if (!SCATTER && c && lane == 0) P.cnt[mt] = c;
    }
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_dm_scan(const LpfDmParams P)
{
    const int fl = blockIdx.y, lane = lpf_lane();
    const int m = blockIdx.x * 4 + lpf_wave();
    if (m >= P.M) return;
    const size_t row = ((size_t)fl * P.M + m) * P.ntile;
    unsigned run = 0;
    for (int t0 = 0; t0 < P.ntile; t0 += 64) {
        const int t = t0 + lane;
        const unsigned v = t < P.ntile ? P.cnt[row + t] : 0u;
        unsigned incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned s = __shfl_up(incl, o);
            if (lane >= o) incl += s;
        }
        if (t < P.ntile) P.toff[row + t] = run + incl - v;
        run += __shfl(incl, 63);
    }
    if (lane == 0) P.tot[(size_t)fl * P.M + m] = run;
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_dm_frame(const LpfDmParams P)
{
    __shared__ unsigned s_tmp[4];
    const int fl = blockIdx.x;
    const size_t fo = (size_t)(P.f0 + fl);
    const int m = threadIdx.x;                                  // M <= 256 = LPF_BLOCK
    const unsigned v = m < P.M ? P.tot[(size_t)fl * P.M + m] : 0u;
    unsigned total;
    const unsigned ex = lpf_wide_block_excl(v, s_tmp, total);
    if (m < P.M) P.car_off[fo * (P.M + 1) + m] = ex;
    if (m == 0) {
        P.car_off[fo * (P.M + 1) + P.M] = total;
        P.need[fo] = total;
        if (P.overflow) P.overflow[fo] = (long long)total > P.cap ? 1 : 0;
    }
}
