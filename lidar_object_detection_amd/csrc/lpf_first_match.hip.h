// lpf_first_match.hip.h -- the exclusive, first-mask-wins labelling of a batch of frames (lpf_first_match, include/lpf.h).
//
// Same_color.py:113-132 walks the valid points of a frame in ascending order and gives each to the FIRST mask m of the frame's list
// with ``y < mask.shape[0] and x < mask.shape[1] and mask[y, x] > 0.5``; a valid point no mask takes is background.  The masks are
// read at their OWN size mh x mw: nothing is resized and nothing outside [0, mh) x [0, mw) is read.  Three launches in stream order
// over a range of frames; no block waits for another.  A block owns a tile of LPF_FM_TILE consecutive points of one frame, four per
// thread (row j, thread t = point j * 256 + t of the tile: the four 16-byte point loads of a lane are in flight together).
//   lpf_fm_count    projects and clips as every projecting kernel does (lpf_project_point, lpf_pixel), then looks for the first mask by
//                   direct reads, LPF_FM_AHEAD masks of every pending row in flight at a time, until no lane of the wave is pending:
//                   lanes leave the loop at different m.  The 4-byte code of every point (-2 not valid, -1 background, else m) goes
//                   to the dense output or to scratch; car and background points are counted per tile with wave ballots;
//                   mask_count[f][m] is gathered in an LDS histogram and sent with ONE integer atomicAdd per (block, non-zero bin)
//                   into an output the call zeroed in stream order.
//   lpf_fm_count_planes   the same for run-length masks (lpf_first_match_rle): the masks are label planes decoded from the runs, and a
//                   point's first mask is the lowest set bit of at most ceil(M / 32) words (at its definition, below).
//   lpf_fm_scan     one block per frame: exclusive prefix of the tile counts, and the frame's n_valid / n_car / n_bg.
//   lpf_fm_scatter  the codes again: a point's slot is its tile's prefix + the counts of the tile's earlier (row, wave) pairs (LDS) +
//                   the popcount of the wave's ballot below its lane, so both lists ascend within the frame.  xyz is gathered from
//                   the points, the colour row from colors[f][m].
// All sums are integers: two runs give the same bytes whatever the order of the blocks.  Entries of a frame's span at or beyond its
// count are not written.  Frame ranges are clamped to [0, 2^31 - 1] points, and a pixel is tested against mh, mw and the image before
// any mask is read.
#pragma once
#include "lpf_kernels.hip.h"
#include "lpf_wide.hip.h"

#define LPF_FM_PER 4                              // points per thread
#define LPF_FM_TILE (LPF_FM_PER * LPF_BLOCK)      // points per block
#define LPF_FM_AHEAD 4                            // masks of a pending row read before the first of them is tested

struct LpfFmParams {
    LpfCam cam;
    const float4 *pts;                      // the range's first point
    int M, mh, mw, f0;                      // masks per frame, their own size, first frame of the range
    long long pt_base;                      // frame_off[f0]: pts and the scratch codes begin there
    long long code_base;                    // code[frame_off[f] + i - code_base]
    long long out_base, fr_base;            // the per-point / per-frame outputs begin at that point / frame (staged ranges; else 0)
    const long long *foff;                  // [F + 1] the batch's frame offsets
    const void *masks;                      // [Fc][M][mh][mw] uint8 or float32, the range's frames; lpf_fm_count_planes: label planes
                                            // [Fc][ceil(M / 32)][mh][mw] uint32
    const double *colors;                   // [Fc][M][3] or null
    int *code;                              // the dense output, or scratch
    int2 *tcnt, *tpre;                      // {car, background} points per tile, their exclusive prefix in the frame: frame f0 + fl's
                                            // tiles from lpf_fm_tile0 on (a range of nc points in fc frames has at most nc / TILE + fc)
    // outputs (nullable), frame f at frame_off[f] - out_base / f - fr_base
    long long *car_idx, *bg_idx;
    int *car_mask;
    float *car_xyz, *bg_xyz;
    double *car_rgb;
    long long *n_valid, *n_car, *n_bg;
    unsigned long long *mask_count;         // [F][M], arrives zeroed
};

// the points of frame f0 + fl: first point in the batch, count (clamped)
__device__ __forceinline__ void lpf_fm_frame(const LpfFmParams &P, const int fl, long long &a, long long &n)
{
    a = P.foff[P.f0 + fl];
    n = P.foff[P.f0 + fl + 1] - a;
    n = n < 0 ? 0 : (n > 0x7fffffffll ? 0x7fffffffll : n);
}

// the first tile of frame f0 + fl, whose first point is a: frames of any sizes get disjoint runs of tiles without a table, since
// floor(x / T) + ceil(n / T) <= floor((x + n) / T) + 1
__device__ __forceinline__ size_t lpf_fm_tile0(const LpfFmParams &P, const int fl, const long long a)
{
    return (size_t)((a - P.pt_base) / LPF_FM_TILE) + (size_t)fl;
}

template <typename T>                       // uint8: nonzero is a member; float: > 0.5 is (NaN, 0.5 and negatives are not)
__global__ __launch_bounds__(LPF_BLOCK) void lpf_fm_count(const LpfFmParams P)
{
    __shared__ unsigned s_hist[LPF_BLOCK];  // M <= 256 = LPF_BLOCK
    __shared__ unsigned s_cnt[2][4];
    constexpr int MODE = sizeof(T) == 1 ? 0 : 3;
    const int fl = blockIdx.y, tid = threadIdx.x, lane = lpf_lane(), wave = lpf_wave();
    long long a, n;
    lpf_fm_frame(P, fl, a, n);
    const long long i0 = (long long)blockIdx.x * LPF_FM_TILE;
    if (i0 >= n) return;
    const int M = P.M, mw = P.mw, mh = P.mh;
    s_hist[tid] = 0u;
    __syncthreads();

    const float4 *__restrict__ pts = P.pts + (a - P.pt_base);
    float4 p[LPF_FM_PER];
#pragma unroll
    for (int j = 0; j < LPF_FM_PER; ++j) {
        const long long i = i0 + j * LPF_BLOCK + tid;
        p[j] = i < n ? pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    int code[LPF_FM_PER];
    long long pix[LPF_FM_PER];              // the pixel's place in a mask plane
    unsigned pend = 0;                      // bit j: row j is valid, inside the masks' own size, and no mask has taken it yet
#pragma unroll
    for (int j = 0; j < LPF_FM_PER; ++j) {
        const long long i = i0 + j * LPF_BLOCK + tid;
        double uf, vf, d;
        int ui, vi;
        lpf_project_point(P.cam, p[j].x, p[j].y, p[j].z, uf, vf, d);
        const bool valid = lpf_pixel(P.cam, uf, vf, d, ui, vi) && i < n;
        code[j] = valid ? -1 : -2;
        pix[j] = 0;
        if (valid && ui < mw && vi < mh) {
            pix[j] = (long long)vi * mw + ui;
            pend |= 1u << j;
        }
    }
    const size_t plane = (size_t)mh * (size_t)mw;
    const T *__restrict__ mk = (const T *)P.masks + (size_t)fl * (size_t)M * plane;
    for (int m0 = 0; m0 < M; m0 += LPF_FM_AHEAD) {
        if (!__ballot(pend != 0u)) break;                     // every lane of the wave is done
        T v[LPF_FM_PER][LPF_FM_AHEAD];
#pragma unroll
        for (int j = 0; j < LPF_FM_PER; ++j)
#pragma unroll
            for (int k = 0; k < LPF_FM_AHEAD; ++k)
                v[j][k] = ((pend >> j) & 1u) ? mk[(size_t)min(m0 + k, M - 1) * plane + pix[j]] : (T)0;
#pragma unroll
        for (int j = 0; j < LPF_FM_PER; ++j)
#pragma unroll
            for (int k = 0; k < LPF_FM_AHEAD; ++k)
                if (((pend >> j) & 1u) && m0 + k < M && lpf_member<T, MODE>(v[j][k])) {
                    code[j] = m0 + k;
                    pend &= ~(1u << j);
                }
    }

    unsigned ncar = 0, nbg = 0;
#pragma unroll
    for (int j = 0; j < LPF_FM_PER; ++j) {
        const long long i = i0 + j * LPF_BLOCK + tid;
        if (i < n) P.code[a + i - P.code_base] = code[j];
        ncar += (unsigned)__popcll(__ballot(code[j] >= 0));
        nbg += (unsigned)__popcll(__ballot(code[j] == -1));
        if (P.mask_count && code[j] >= 0) atomicAdd(&s_hist[code[j]], 1u);
    }
    if (lane == 0) { s_cnt[0][wave] = ncar; s_cnt[1][wave] = nbg; }
    __syncthreads();
    if (tid == 0)
        P.tcnt[lpf_fm_tile0(P, fl, a) + blockIdx.x] = make_int2((int)(s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3]),
                                                                   (int)(s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3]));
    if (P.mask_count && tid < M && s_hist[tid])
        atomicAdd(&P.mask_count[(size_t)(P.f0 + fl - P.fr_base) * M + tid], (unsigned long long)s_hist[tid]);
}

// lpf_fm_count for run-length masks (lpf_first_match_rle): P.masks are the range's label planes [Fc][LW][mh][mw] uint32, LW =
// ceil(M / 32), bit m & 31 of plane m / 32 = mask m (zeroed, then lpf_rle_decode_wide).  The same tile, projection, clip, pend logic,
// code store, ballots, histogram and atomics as lpf_fm_count -- kept word for word, so that the two stay comparable line by line; only
// the walk differs: a pending row reads word w of its pixel, LPF_FM_AHEAD words in flight before the first is tested, and its code is
// 32 w + the lowest set bit of the first nonzero word: at most LW <= 8 reads where the dense walk makes up to M.  Bits at or above M
// are zero by construction, but nothing relies on it: a code >= M leaves the point background (and ends its walk: no lower mask has
// it), so s_hist and mask_count are never indexed past M.
__global__ __launch_bounds__(LPF_BLOCK) void lpf_fm_count_planes(const LpfFmParams P)
{
    __shared__ unsigned s_hist[LPF_BLOCK];  // M <= 256 = LPF_BLOCK
    __shared__ unsigned s_cnt[2][4];
    const int fl = blockIdx.y, tid = threadIdx.x, lane = lpf_lane(), wave = lpf_wave();
    long long a, n;
    lpf_fm_frame(P, fl, a, n);
    const long long i0 = (long long)blockIdx.x * LPF_FM_TILE;
    if (i0 >= n) return;
    const int M = P.M, mw = P.mw, mh = P.mh, LW = (M + 31) >> 5;
    s_hist[tid] = 0u;
    __syncthreads();

    const float4 *__restrict__ pts = P.pts + (a - P.pt_base);
    float4 p[LPF_FM_PER];
#pragma unroll
    for (int j = 0; j < LPF_FM_PER; ++j) {
        const long long i = i0 + j * LPF_BLOCK + tid;
        p[j] = i < n ? pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    int code[LPF_FM_PER];
    long long pix[LPF_FM_PER];              // the pixel's place in a plane
    unsigned pend = 0;                      // bit j: row j is valid, inside the masks' own size, and no mask has taken it yet
#pragma unroll
    for (int j = 0; j < LPF_FM_PER; ++j) {
        const long long i = i0 + j * LPF_BLOCK + tid;
        double uf, vf, d;
        int ui, vi;
        lpf_project_point(P.cam, p[j].x, p[j].y, p[j].z, uf, vf, d);
        const bool valid = lpf_pixel(P.cam, uf, vf, d, ui, vi) && i < n;
        code[j] = valid ? -1 : -2;
        pix[j] = 0;
        if (valid && ui < mw && vi < mh) {
            pix[j] = (long long)vi * mw + ui;
            pend |= 1u << j;
        }
    }
    const size_t plane = (size_t)mh * (size_t)mw;
    const uint32_t *__restrict__ pl = (const uint32_t *)P.masks + (size_t)fl * (size_t)LW * plane;
    for (int w0 = 0; w0 < LW; w0 += LPF_FM_AHEAD) {
        if (!__ballot(pend != 0u)) break;                     // every lane of the wave is done
        uint32_t v[LPF_FM_PER][LPF_FM_AHEAD];
#pragma unroll
        for (int j = 0; j < LPF_FM_PER; ++j)
#pragma unroll
            for (int k = 0; k < LPF_FM_AHEAD; ++k)
                v[j][k] = ((pend >> j) & 1u) ? pl[(size_t)min(w0 + k, LW - 1) * plane + pix[j]] : 0u;
#pragma unroll
        for (int j = 0; j < LPF_FM_PER; ++j)
#pragma unroll
            for (int k = 0; k < LPF_FM_AHEAD; ++k)
                if (((pend >> j) & 1u) && w0 + k < LW && v[j][k]) {
                    const int m = 32 * (w0 + k) + (__ffs((int)v[j][k]) - 1);
                    if (m < M) code[j] = m;
                    pend &= ~(1u << j);
                }
    }

    unsigned ncar = 0, nbg = 0;
#pragma unroll
    for (int j = 0; j < LPF_FM_PER; ++j) {
        const long long i = i0 + j * LPF_BLOCK + tid;
        if (i < n) P.code[a + i - P.code_base] = code[j];
        ncar += (unsigned)__popcll(__ballot(code[j] >= 0));
        nbg += (unsigned)__popcll(__ballot(code[j] == -1));
        if (P.mask_count && code[j] >= 0) atomicAdd(&s_hist[code[j]], 1u);
    }
    if (lane == 0) { s_cnt[0][wave] = ncar; s_cnt[1][wave] = nbg; }
    __syncthreads();
    if (tid == 0)
        P.tcnt[lpf_fm_tile0(P, fl, a) + blockIdx.x] = make_int2((int)(s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3]),
                                                                   (int)(s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3]));
    if (P.mask_count && tid < M && s_hist[tid])
        atomicAdd(&P.mask_count[(size_t)(P.f0 + fl - P.fr_base) * M + tid], (unsigned long long)s_hist[tid]);
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_fm_scan(const LpfFmParams P)
{
    __shared__ unsigned s_tmp[8];
    const int fl = blockIdx.x, tid = threadIdx.x;
    long long a, n;
    lpf_fm_frame(P, fl, a, n);
    const int ntile = (int)((n + LPF_FM_TILE - 1) / LPF_FM_TILE);
    const size_t row = lpf_fm_tile0(P, fl, a);
    unsigned run_c = 0, run_b = 0;
    for (int t0 = 0; t0 < ntile; t0 += LPF_BLOCK) {
        const int t = t0 + tid;
        const int2 v = t < ntile ? P.tcnt[row + t] : make_int2(0, 0);
        unsigned tc, tb;
        const unsigned ec = lpf_wide_block_excl((unsigned)v.x, s_tmp, tc);
        const unsigned eb = lpf_wide_block_excl((unsigned)v.y, s_tmp + 4, tb);
        if (t < ntile) P.tpre[row + t] = make_int2((int)(run_c + ec), (int)(run_b + eb));
        run_c += tc; run_b += tb;
    }
    if (tid == 0) {
        const size_t fo = (size_t)(P.f0 + fl - P.fr_base);
        if (P.n_valid) P.n_valid[fo] = (long long)run_c + (long long)run_b;
        P.n_car[fo] = run_c;
        P.n_bg[fo] = run_b;
    }
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_fm_scatter(const LpfFmParams P)
{
    __shared__ unsigned s_cnt[2][LPF_FM_PER * 4];            // [car | background][row * 4 + wave]
    const int fl = blockIdx.y, tid = threadIdx.x, lane = lpf_lane(), wave = lpf_wave();
    long long a, n;
    lpf_fm_frame(P, fl, a, n);
    const long long i0 = (long long)blockIdx.x * LPF_FM_TILE;
    if (i0 >= n) return;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int code[LPF_FM_PER];
    unsigned below[LPF_FM_PER];             // the wave's points of the same kind in lower lanes of the row
#pragma unroll
    for (int j = 0; j < LPF_FM_PER; ++j) {
        const long long i = i0 + j * LPF_BLOCK + tid;
        code[j] = i < n ? P.code[a + i - P.code_base] : -2;
    }
#pragma unroll
    for (int j = 0; j < LPF_FM_PER; ++j) {
        const unsigned long long bc = __ballot(code[j] >= 0), bb = __ballot(code[j] == -1);
        below[j] = (unsigned)__popcll((code[j] >= 0 ? bc : bb) & lt);
        if (lane == 0) { s_cnt[0][j * 4 + wave] = (unsigned)__popcll(bc); s_cnt[1][j * 4 + wave] = (unsigned)__popcll(bb); }
    }
    __syncthreads();
    const int2 pre = P.tpre[lpf_fm_tile0(P, fl, a) + blockIdx.x];
    const float4 *__restrict__ pts = P.pts + (a - P.pt_base);
    const size_t o0 = (size_t)(a - P.out_base);
    const int M = P.M;
#pragma unroll
    for (int j = 0; j < LPF_FM_PER; ++j) {
        if (code[j] < -1) continue;
        const int kind = code[j] >= 0 ? 0 : 1;
        unsigned before = 0;
        for (int q = 0; q < j * 4 + wave; ++q) before += s_cnt[kind][q];
        const long long i = i0 + j * LPF_BLOCK + tid;
        const size_t o = o0 + (size_t)(kind ? pre.y : pre.x) + before + below[j];
        if (kind == 0) {
            if (P.car_idx) P.car_idx[o] = i;
            if (P.car_mask) P.car_mask[o] = code[j];
            if (P.car_xyz) {
                const float4 q = pts[i];
                P.car_xyz[3 * o] = q.x; P.car_xyz[3 * o + 1] = q.y; P.car_xyz[3 * o + 2] = q.z;
            }
            if (P.car_rgb && code[j] < M) {
                const double *__restrict__ c = P.colors + ((size_t)fl * M + code[j]) * 3;
                P.car_rgb[3 * o] = c[0]; P.car_rgb[3 * o + 1] = c[1]; P.car_rgb[3 * o + 2] = c[2];
            }
        } else {
            if (P.bg_idx) P.bg_idx[o] = i;
            if (P.bg_xyz) {
                const float4 q = pts[i];
                P.bg_xyz[3 * o] = q.x; P.bg_xyz[3 * o + 1] = q.y; P.bg_xyz[3 * o + 2] = q.z;
            }
        }
    }
}
