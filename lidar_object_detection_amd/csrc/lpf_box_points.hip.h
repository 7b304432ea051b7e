// lpf_box_points.hip.h -- per-box LiDAR point counts and the first box of every valid point of a batch (lpf_box_points, include/lpf.h).
//
// The counting kernels test the MASKED points of a frame against its boxes (count_mb: the numerators of a recall); the denominator is
// the box test of V3:167-208 / V3:143-164 on ALL of points_valid (V3:590-592).  After a run the compacted valid indices, the compact
// label words, the points and the packed box parameters are in HBM: one launch gives, per box, the valid points it holds and how many
// of them carry a label bit; per valid point, the first box that holds it; per frame, the four counts of the point-level confusion
// matrix.
//
// One launch: grid (chunks of LPF_BP_CHUNK compact entries of the frame with the most, frames), point-major.  A block owns 1024
// consecutive entries of one frame, four per thread (entry e0 + j * 256 + tid: the four index loads, then the four 16-byte point
// gathers of a thread are in flight together; the indices ascend, so neighbouring lanes hit neighbouring sectors), and keeps them in
// registers while the frame's boxes pass through LDS in tiles of LPF_BP_TILE = 64 (boxp 8 KB + the six float bounds of boxq):
//   - every lane of a wave tests its four points against the SAME box j, so the box reads are LDS broadcasts and the loop is
//     wave-uniform: the float-bounds reject on boxq first, then lpf_oriented_inside / lpf_aabb_inside on boxp, exactly as
//     lpf_wide_boxes_block applies them -- so count_mb[m][b] <= box_labelled[b] <= box_points[b] holds bit for bit;
//   - per (wave, box, row) two ballots (inside; inside and labelled) and two popcounts; lane j keeps box j's two sums in registers for
//     the tile; the four waves' sums meet in LDS and ONE global integer atomicAdd per (block, box) with a non-zero sum goes into the
//     output, which the call zeroed in stream order;
//   - first_box is a per-thread running minimum: the first j that hits, since tiles and boxes are met in ascending order; no atomics;
//   - frame_counts[f][1..3] go the same way as the box sums (ballots, LDS, one atomicAdd per block and count); [0] is the frame's
//     clamped n_valid, stored by the frame's first block.
// All sums are integers: the same bytes every run, whatever the order of the blocks.  Nothing is read or written out of bounds
// whatever the lists hold: n_valid[f] is clamped to [0, N_f], an entry whose index is outside the frame's points is tested against
// nothing (first_box -1, counted only in frame_counts[f][0]).
#pragma once
#include "lpf_kernels.hip.h"

#define LPF_BP_PER 4                              // entries per thread
#define LPF_BP_CHUNK (LPF_BP_PER * LPF_BLOCK)     // entries per block
#define LPF_BP_TILE 64                            // boxes per LDS tile: one per lane of a wave

struct LpfBpParams {
    const LpfBatchFrame *frames;    // frame f0 + blockIdx.y
    const float4 *pts;
    const long long *valid_idx;   // [Ntot] compact
    const long long *n_valid;     // [F]
    const uint32_t *labels;       // [Ntot][LW] compact; null: nothing is labelled
    const double *boxp;           // [Btot][16] the packed box parameters in force
    const float *boxq;            // [Btot][8] their float bounds {lo xyz, -, hi xyz, -}
    int LW, f0;
    int *box_points;              // null: not wanted (each of the four); the two box arrays and frame_counts arrive zeroed
    int *box_labelled;
    int *first_box;
    long long *frame_counts;      // [F][4]
};

template <bool ORIENTED>          // the boxes in force are oriented (lpf_oriented_inside) or axis-aligned hulls (lpf_aabb_inside)
__global__ __launch_bounds__(LPF_BLOCK) void lpf_box_points_kernel(const LpfBpParams Q)
{
    __shared__ double s_bp[LPF_BP_TILE * 16];
    __shared__ float s_bq[LPF_BP_TILE * 6];
    __shared__ unsigned s_sum[2][4][LPF_BP_TILE];      // [points | labelled][wave][box of the tile]
    __shared__ unsigned s_fc[3][4];                    // [in a box | labelled | both][wave]
    const int f = Q.f0 + (int)blockIdx.y;
    const int tid = threadIdx.x, lane = lpf_lane(), wave = lpf_wave();
    const LpfBatchFrame fr = Q.frames[f];
    const long long nv = Q.n_valid[f];
    const int n = nv < 0 ? 0 : (nv > (long long)fr.N ? fr.N : (int)nv);
    if (blockIdx.x == 0 && tid == 0 && Q.frame_counts) Q.frame_counts[(size_t)f * 4] = n;
    // (entries are counted in 64 bits: a frame may have up to 2^31 - 1 points, and e0 + 1023 may pass that)
    const long long e0 = (long long)blockIdx.x * LPF_BP_CHUNK;
    if (e0 >= (long long)n) return;
    const float4 *__restrict__ P = Q.pts + fr.pt_off;
    const long long *__restrict__ list = Q.valid_idx + fr.pt_off;

    long long idx[LPF_BP_PER];
    float4 x[LPF_BP_PER];
    int first[LPF_BP_PER];
    unsigned okm = 0, labm = 0;                        // bit j: entry of row j has a point of the frame / carries a label bit
#pragma unroll
    for (int j = 0; j < LPF_BP_PER; ++j) {
        const long long e = e0 + j * LPF_BLOCK + tid;
        idx[j] = e < (long long)n ? list[e] : -1;
    }
#pragma unroll
    for (int j = 0; j < LPF_BP_PER; ++j) {
        const bool ok = (unsigned long long)idx[j] < (unsigned long long)fr.N;     // (also false for the -1 of a row beyond the list)
        x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) x[j] = P[idx[j]];
        okm |= (ok ? 1u : 0u) << j;
        first[j] = -1;
    }
    if (Q.labels && Q.LW > 0) {
#pragma unroll
        for (int j = 0; j < LPF_BP_PER; ++j) {
            if (!((okm >> j) & 1u)) continue;
            const uint32_t *__restrict__ w = Q.labels + (size_t)(fr.pt_off + e0 + j * LPF_BLOCK + tid) * (size_t)Q.LW;
            uint32_t any = 0;
            for (int k = 0; k < Q.LW; ++k) any |= w[k];
            labm |= (any ? 1u : 0u) << j;
        }
    }

    for (int b0 = 0; b0 < fr.B; b0 += LPF_BP_TILE) {
        const int nb = min(LPF_BP_TILE, fr.B - b0);
        const double *__restrict__ bp = Q.boxp + ((size_t)fr.box_off + b0) * 16;
        const float *__restrict__ bq = Q.boxq + ((size_t)fr.box_off + b0) * 8;
        __syncthreads();                               // the tile before has been read, its sums sent
        for (int i = tid; i < nb * 16; i += LPF_BLOCK) s_bp[i] = bp[i];
        for (int i = tid; i < nb * 6; i += LPF_BLOCK) { const int bx = i / 6, k = i - 6 * bx; s_bq[i] = bq[8 * bx + (k < 3 ? k : k + 1)]; }
        __syncthreads();
        unsigned cp = 0, cl = 0;                       // lane j: box b0 + j's points / labelled points among this wave's entries
        for (int j = 0; j < nb; ++j) {
            const float *q = s_bq + 6 * j;
            const float q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], q5 = q[5];
            unsigned np_ = 0, nl_ = 0;
#pragma unroll
            for (int r = 0; r < LPF_BP_PER; ++r) {
                const float4 p = x[r];
                bool in = false;
                if (((okm >> r) & 1u) && p.x >= q0 && p.x <= q3 && p.y >= q1 && p.y <= q4 && p.z >= q2 && p.z <= q5) {
                    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
                    in = ORIENTED ? lpf_oriented_inside(px, py, pz, s_bp + 16 * j) : lpf_aabb_inside(px, py, pz, s_bp + 16 * j);
                }
                if (in && first[r] < 0) first[r] = b0 + j;
                np_ += (unsigned)__popcll(__ballot(in));
                nl_ += (unsigned)__popcll(__ballot(in && ((labm >> r) & 1u)));
            }
            if (lane == j) { cp = np_; cl = nl_; }
        }
        s_sum[0][wave][lane] = cp;
        s_sum[1][wave][lane] = cl;
        __syncthreads();
        if (tid < 2 * LPF_BP_TILE) {
            const int which = tid >> 6, j = tid & 63;
            const unsigned v = s_sum[which][0][j] + s_sum[which][1][j] + s_sum[which][2][j] + s_sum[which][3][j];
            int *__restrict__ dst = which ? Q.box_labelled : Q.box_points;
            if (v && j < nb && dst) atomicAdd(&dst[(size_t)fr.box_off + b0 + j], (int)v);
        }
    }

    unsigned nbx = 0, nlb = 0, nbo = 0;                // this wave's entries in a box / labelled / both
#pragma unroll
    for (int j = 0; j < LPF_BP_PER; ++j) {
        const bool ok = (okm >> j) & 1u, lab = (labm >> j) & 1u, boxed = first[j] >= 0;
        nbx += (unsigned)__popcll(__ballot(ok && boxed));
        nlb += (unsigned)__popcll(__ballot(ok && lab));
        nbo += (unsigned)__popcll(__ballot(ok && lab && boxed));
        const long long e = e0 + j * LPF_BLOCK + tid;
        if (Q.first_box && e < (long long)n) Q.first_box[(size_t)(fr.pt_off + e)] = first[j];
    }
    if (!Q.frame_counts) return;
    if (lane == 0) { s_fc[0][wave] = nbx; s_fc[1][wave] = nlb; s_fc[2][wave] = nbo; }
    __syncthreads();
    if (tid < 3) {
        const unsigned v = s_fc[tid][0] + s_fc[tid][1] + s_fc[tid][2] + s_fc[tid][3];
        if (v) atomicAdd((unsigned long long *)Q.frame_counts + (size_t)f * 4 + 1 + tid, (unsigned long long)v);
    }
}
