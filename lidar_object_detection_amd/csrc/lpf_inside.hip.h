// lpf_inside.hip.h -- V3's per-car inside / outside split of a batch of frames (lpf_inside_masks, include/lpf.h).
//
// V3:386-398 stores, for a car that found its box, inside_mask = oriented_point_in_bbox(car_points, best box) next to car_points, and
// create_colored_point_cloud_with_bbox_analysis (V3:471-515) shows car_points[inside_mask] and car_points[~inside_mask]; a car without a
// box (V3:413-425) keeps inside_mask = None.  After a run the instance lists, the best box per car and the packed box parameters are all
// in HBM: ONE box test per list entry gives the mask and the two parts, for every car of every frame, in one launch.
//
// One launch: grid (cars, frames), a block per car.  Why a block: a car has between 0 and tens of thousands of entries and the order of
// the two parts is the list's, so a car is walked front to back with a running count of the entries found inside -- a block takes
// LPF_IN_STEP = 1024 entries per step (four per thread, the four index loads and the four 16-byte point gathers of a thread in flight
// together), which keeps the longest car to a few dozen steps where a single wave would need hundreds, and the many small cars (most have
// fewer than 1024 points) are one step of a block that then ends; empty and unmatched cars cost a block that copies or returns.  Nothing
// is shared between blocks, so there is no atomic, no second pass and no dependence on the order in which blocks run:
//   - the car's 16 box doubles (the table the counting kernels read: lpf_oriented_inside / lpf_aabb_inside) go through LDS once and
//     stay in registers;
//   - entry e of the car is tested by thread e % 256 of the step's row e / 256 % 4; a wave's ballot gives the rank of an entry among the
//     wave's, the 16 wave counts of the step (LDS, two sets in turn: one barrier per step) give the ranks before the wave;
//   - the outside part starts at inst_off + best_cnt, known before any test runs: an inside entry goes to inst_off + (inside entries
//     before it), an outside one to inst_off + best_cnt + (outside entries before it).  Both parts keep the list's ascending order.
// The test is the one that produced best_cnt, on the same parameters, so the entries found inside number best_cnt; should the caller's
// best_cnt not be that count, the parts stay within the car's entries all the same (a position outside them is not written).  Nothing is
// read or written out of bounds whatever the arrays hold: offsets that do not ascend within [0, inst_cap] skip the car, an index outside
// the frame's points is an outside entry with zero coordinates, a best box outside the frame's boxes is no box.
#pragma once
#include "lpf_kernels.hip.h"

#define LPF_IN_PER 4                              // entries per thread and step
#define LPF_IN_STEP (LPF_IN_PER * LPF_BLOCK)      // entries per block and step

struct LpfInParams {
    const LpfBatchFrame *frames;    // frame f0 + blockIdx.y
    const float4 *pts;
    const long long *inst_idx;    // [F][inst_cap]
    long long inst_cap;
    const long long *inst_off;    // [F][M + 1]
    const int *best_box;          // [F][M]
    const long long *best_cnt;    // [F][M]
    const double *boxp;           // [Btot][16] the packed box parameters in force
    int M, min_points, f0, pad;
    unsigned char *inside;        // null: not wanted (each of the five)
    long long *part_idx;
    float *part_xyz;
    long long *n_inside;
    int *matched;
};

template <bool ORIENTED>          // the boxes in force are oriented (lpf_oriented_inside) or axis-aligned hulls (lpf_aabb_inside)
__global__ __launch_bounds__(LPF_BLOCK) void lpf_inside_cars(const LpfInParams Q)
{
    __shared__ double s_box[16];
    __shared__ unsigned s_wc[2][LPF_IN_PER * 4];
    const int m = blockIdx.x, f = Q.f0 + (int)blockIdx.y;
    const int tid = threadIdx.x, lane = lpf_lane(), wave = lpf_wave();
    const LpfBatchFrame fr = Q.frames[f];
    const size_t car = (size_t)f * Q.M + m;
    const long long *__restrict__ off = Q.inst_off + (size_t)f * (Q.M + 1);
    const long long o0 = off[m], o1 = off[m + 1], tot = off[Q.M];
    const int bb = Q.best_box[car];
    const long long bc = Q.best_cnt[car];
    const bool matched = bb >= 0 && bb < fr.B && bc >= (long long)Q.min_points;
    // (a frame whose lists did not fit has inst_off[M] > inst_cap: its rows are left alone)
    const bool lists = o0 >= 0 && o0 <= o1 && o1 <= tot && tot <= Q.inst_cap;
    // (32-bit counts below: a list holds a point of its frame at most once, and a frame has fewer than 2^31 - LPF_IN_STEP points)
    const int k = (lists && o1 - o0 <= 0x7fffffffll - LPF_IN_STEP) ? (int)(o1 - o0) : 0;
    if (tid == 0 && Q.matched) Q.matched[car] = matched ? 1 : 0;
    if (k == 0 || !(Q.inside || Q.part_idx || Q.part_xyz || (Q.n_inside && matched))) {
        if (tid == 0 && Q.n_inside) Q.n_inside[car] = 0;
        return;
    }

    double b[16];
    if (matched) {
        if (tid < 16) s_box[tid] = Q.boxp[((size_t)fr.box_off + bb) * 16 + tid];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = s_box[i];
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = 0.0;
    }
    const int nin = matched ? (int)(bc < (long long)k ? bc : (long long)k) : 0;     // where the outside part starts
    const size_t row = (size_t)f * (size_t)Q.inst_cap + (size_t)o0;     // the car's first entry in the [F][inst_cap] arrays
    const long long *__restrict__ list = Q.inst_idx + row;
    unsigned char *__restrict__ o_in = Q.inside ? Q.inside + row : nullptr;
    long long *__restrict__ o_idx = Q.part_idx ? Q.part_idx + row : nullptr;
    float *__restrict__ o_xyz = Q.part_xyz ? Q.part_xyz + row * 3 : nullptr;
    const float4 *__restrict__ P = Q.pts + fr.pt_off;
    const unsigned long long lt = (1ull << lane) - 1ull;

    int run = 0;                                                         // inside entries before this step
    int par = 0;
    for (int e0 = 0; e0 < k; e0 += LPF_IN_STEP, par ^= 1) {
        long long idx[LPF_IN_PER];
        float4 x[LPF_IN_PER];
        unsigned inm = 0;                                                // bit j: entry of row j lies inside
        unsigned rank[LPF_IN_PER];
#pragma unroll
        for (int j = 0; j < LPF_IN_PER; ++j) {
            const int e = e0 + j * LPF_BLOCK + tid;
            idx[j] = e < k ? list[e] : -1;
        }
#pragma unroll
        for (int j = 0; j < LPF_IN_PER; ++j) {
            const bool ok = (unsigned long long)idx[j] < (unsigned long long)fr.N;    // (also false for the -1 of a row beyond the car)
            x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) x[j] = P[idx[j]];
        }
#pragma unroll
        for (int j = 0; j < LPF_IN_PER; ++j) {
            const bool ok = (unsigned long long)idx[j] < (unsigned long long)fr.N;    // (also false for the -1 of a row beyond the car)
            bool in = false;
            if (matched && ok) {
                const double px = (double)x[j].x, py = (double)x[j].y, pz = (double)x[j].z;
                in = ORIENTED ? lpf_oriented_inside(px, py, pz, b) : lpf_aabb_inside(px, py, pz, b);
            }
            inm |= (in ? 1u : 0u) << j;
            const unsigned long long bal = __ballot(in);
            rank[j] = (unsigned)__popcll(bal & lt);
            if (lane == 0) s_wc[par][j * 4 + wave] = (unsigned)__popcll(bal);
        }
        __syncthreads();
        unsigned before[LPF_IN_PER], total = 0;                         // inside entries of the step before row j of this wave
#pragma unroll
        for (int j = 0; j < LPF_IN_PER; ++j) before[j] = 0;
#pragma unroll
        for (int q = 0; q < LPF_IN_PER * 4; ++q) {
            const unsigned c = s_wc[par][q];
#pragma unroll
            for (int j = 0; j < LPF_IN_PER; ++j)
                if (q < j * 4 + wave) before[j] += c;
            total += c;
        }
#pragma unroll
        for (int j = 0; j < LPF_IN_PER; ++j) {
            const int e = e0 + j * LPF_BLOCK + tid;
            if (e >= k) continue;
            const int ins = run + (int)(before[j] + rank[j]);           // inside entries of the car before entry e
            const bool in = (inm >> j) & 1u;
            const int pos = in ? ins : nin + (e - ins);
            if (o_in) o_in[e] = in ? 1 : 0;
            if (in ? pos < nin : pos < k) {
                if (o_idx) o_idx[pos] = idx[j];
                if (o_xyz) {
                    float *__restrict__ o = o_xyz + (size_t)pos * 3;
                    o[0] = x[j].x; o[1] = x[j].y; o[2] = x[j].z;
                }
            }
        }
        run += total;
    }
    if (tid == 0 && Q.n_inside) Q.n_inside[car] = run;
}
