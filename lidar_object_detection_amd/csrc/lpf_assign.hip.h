// lpf_assign.hip.h -- V5's Hungarian assignment for a batch of frames (lpf_assign_costs, lpf_assign_2d, include/lpf.h).
//
// V5:307-416 (improved_match_detections_to_bboxes) hands its cost matrix, without the columns of boxes that have no projection
// (V5:337-341), to scipy.optimize.linear_sum_assignment.  The result the reference shows is SciPy's choice among equally good
// assignments, and V5's costs tie often, so the solver here is SciPy's algorithm statement for statement: the rectangular LSAP by
// shortest augmenting paths with duals, on the transpose when the matrix is tall.  For nr <= nc:
//   u = 0, v = 0, col4row = -1, row4col = -1
//   for cur = 0 .. nr - 1:  minVal = 0, i = cur, spc = +inf, remaining[it] = nc - 1 - it (DESCENDING), n_rem = nc, then until a sink:
//     SR[i] = 1;  for it < n_rem, j = remaining[it]:  r = ((minVal + cost[i][j]) - u[i]) - v[j] (float64, separate operations, this
//     order);  r < spc[j]: spc[j] = r, path[j] = i;  index = the argmin below;  minVal = spc[remaining[index]], +inf: infeasible;
//     j = remaining[index];  row4col[j] == -1: j is the sink, else i = row4col[j];  SC[j] = 1;  remaining[index] = remaining[--n_rem]
//     u[cur] += minVal;  SR[i], i != cur: u[i] += minVal - spc[col4row[i]];  SC[j]: v[j] -= minVal - spc[j]
//     j = sink;  loop { i = path[j]; row4col[j] = i; swap(col4row[i], j) } until i == cur
// The argmin: among the positions whose spc equals the minimum, the LAST one whose column is free (row4col == -1); if none is free,
// the FIRST one.  That is the closed form of SciPy's sequential scan `spc < lowest || (spc == lowest && row4col[j] == -1)` -- a lower
// value always takes over, an equal one only with a free column -- and it is a total order on (value, free, position), so a wave
// reduction computes it whatever order the lanes meet the positions in (lpf_as_better).  tests/assign_ref.py is the same in Python.
//
// Three kernels per range of frames, in stream order:
//   lpf_as_pack    grid (row groups, frames), as lpf_m2_pairs: the frame's live columns (front > 0, or all) are numbered by a block
//                  scan; the block's LPF_M2_ROWS rows of the cost matrix -- copied from the caller's, or scored by lpf_m2_pair, the
//                  device function lpf_match_2d's kernel calls -- are written to the scratch matrix with the live columns only,
//                  TRANSPOSED when the frame is tall (fewer live columns than rows), so that the solver's rows are contiguous.  A NaN
//                  or -inf among them sets the frame's status to 1 (SciPy: "matrix contains invalid numeric entries").
//   lpf_as_solve   one workgroup of ONE wave per frame.  u, v, spc, path, row4col, col4row, remaining and the SR / SC flags live in
//                  LDS: (8 + 8 + 4 + 4 + 4 + 1) bytes per column, (8 + 4 + 1) per row, 42 KB at LPF_ASSIGN_MAX = 1024.  A step is one
//                  dependent row read, nc / 64 <= 16 values per lane, the LDS update and one wave argmin; a chain of latencies that block
//                  barriers would only lengthen, so the batch supplies the parallelism: a frame per CU.  (__syncthreads() of a one-wave
//                  workgroup is the LDS fence between the lanes' writes and reads, no wait for another wave.)
//   lpf_as_finish  (lpf_assign_2d) one block per frame: every assigned pair scored again by lpf_m2_pair, so that the four scores are
//                  lpf_match_2d's bits; accepted = total >= min_score && iou >= min_iou (V5:368).
//
// Termination and bounds (the frames may be anything, the memory lent): the search of a path is a loop of at most nc steps -- a step
// removes one column from `remaining` -- and there are nr paths; the augmenting walk is a loop of at most nr + 1 steps.  Every index read
// from LDS is checked against its range before it is used; a minimum that is not below +inf (no column can be reached, or NaN reached
// the duals) ends the frame with status 2, "cost matrix is infeasible".  Nothing is read or written outside the frame's rows, columns
// and scratch block whatever the values are.
#pragma once
#include "lpf_match2d.hip.h"
#include <type_traits>

#define LPF_AS_CAP 1024           // = LPF_ASSIGN_MAX (include/lpf.h): rows and live columns of a frame

struct LpfAsParams {
    const LpfM2Frame *frames;     // the range's frames: frame blockIdx.y (pack) / blockIdx.x (solve, finish)
    const double *cost;           // lpf_assign_costs: the caller's [P] matrices; pair p at cost + (p - pair_base)
    const void *dets;             // lpf_assign_2d: as LpfM2Params
    const double *bbox2d;
    const int *front;             // null: every column is live
    int det_base, box_base;
    long long pair_base;
    double *scratch;              // the range's matrices of live columns: frame f's at scratch + (p0 - scr_pair_base)
    int *colmap;                  // live column k of frame f -> its box: colmap[b0 - scr_box_base + k]
    int *nlive;                   // [frames of the range]
    long long scr_pair_base;
    int scr_box_base;
    int *col;                     // col_of_row / box_of_det; detection d at col + (d - col_base)
    int *status;                  // [frames of the range]
    int col_base, score_base;
    double *iou, *center, *size, *total;   // lpf_assign_2d, null: not wanted; detection d at + (d - score_base)
    int *accepted;
    double w_iou, w_center, w_size, min_score, min_iou;
};

// MODE 0: the caller's cost matrix;  1 / 2: scored from float / double detections
template <int MODE>
__global__ __launch_bounds__(LPF_BLOCK) void lpf_as_pack(const LpfAsParams Q)
{
    using T = typename std::conditional<MODE == 2, double, float>::type;
    constexpr int NB = MODE ? LPF_AS_CAP : 1;
    __shared__ int s_map[LPF_AS_CAP];
    __shared__ int s_cnt[4];
    __shared__ double s_x0[NB], s_y0[NB], s_x1[NB], s_y1[NB];
    const LpfM2Frame fr = Q.frames[blockIdx.y];
    const int row0 = (int)blockIdx.x * LPF_M2_ROWS;
    if (blockIdx.x != 0 && row0 >= fr.D) return;                          // (the whole block: the grid is sized by the largest frame)
    const int tid = threadIdx.x, lane = lpf_lane(), wave = lpf_wave();
    const int B = fr.B, D = fr.D;

    // the live columns in ascending order: s_map[k], k < nl (never more than the cap: the host refuses such a frame where it can count)
    int nl = 0;
    for (int c0 = 0; c0 < B; c0 += LPF_BLOCK) {
        const int j = c0 + tid;
        const bool live = j < B && (!Q.front || Q.front[(long long)fr.b0 + j - Q.box_base] > 0);
        const unsigned long long m = __ballot(live);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int before = nl;
        for (int w = 0; w < wave; ++w) before += s_cnt[w];
        const int k = before + __popcll(m & ((1ull << lane) - 1ull));
        if (live && k < LPF_AS_CAP) s_map[k] = j;
        nl += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        __syncthreads();
    }
    nl = min(nl, LPF_AS_CAP);
    if (blockIdx.x == 0) {
        for (int k = tid; k < nl; k += LPF_BLOCK) Q.colmap[(long long)fr.b0 - Q.scr_box_base + k] = s_map[k];
        if (tid == 0) Q.nlive[blockIdx.y] = nl;
    }
    if (row0 >= D || nl == 0) return;
    if (MODE) {
        for (int k = tid; k < nl; k += LPF_BLOCK) {
            const double *q = Q.bbox2d + ((long long)fr.b0 + s_map[k] - Q.box_base) * 4;
            s_x0[k] = q[0]; s_y0[k] = q[1]; s_x1[k] = q[2]; s_y1[k] = q[3];
        }
        __syncthreads();
    }

    constexpr int RPW = LPF_M2_ROWS / 4;
    const bool tall = nl < D;
    double *const S = Q.scratch + (fr.p0 - Q.scr_pair_base);
    bool bad = false;
    for (int r = 0; r < RPW; ++r) {
        const int d = row0 + wave * RPW + r;
        if (d >= D) break;                                                 // wave-uniform
        T x1 = (T)0, y1 = (T)0, x2 = (T)0, y2 = (T)0, ar = (T)0, cx = (T)0, cy = (T)0;
        if (MODE) {                                                        // the detection, as lpf_m2_pairs prepares it
            const T *p = (const T *)Q.dets + ((long long)fr.d0 + d - Q.det_base) * 4;
            x1 = p[0]; y1 = p[1]; x2 = p[2]; y2 = p[3];
            ar = (x2 - x1) * (y2 - y1);
            cx = (x1 + x2) / (T)2; cy = (y1 + y2) / (T)2;
        }
        for (int k = lane; k < nl; k += 64) {
            double cost;
            if (MODE) {
                const double q0 = s_x0[k], q1 = s_y0[k], q2 = s_x1[k], q3 = s_y1[k];
                double iou = 0.0, cs = 0.0, ss = 0.0, st = 0.0;
                lpf_m2_pair<T, true>(x1, y1, x2, y2, ar, cx, cy, q0, q1, q2, q3, (q0 + q2) / 2.0, (q1 + q3) / 2.0, (q2 - q0) * (q3 - q1),
                                     Q.w_size, iou, cs, ss, st);
                cost = 1.0 - ((Q.w_iou * iou + Q.w_center * cs) + st);
            } else {
                cost = Q.cost[fr.p0 + (long long)d * B + s_map[k] - Q.pair_base];
            }
            bad |= cost != cost || cost == -INFINITY;
            S[tall ? (long long)k * D + d : (long long)d * nl + k] = cost;
        }
    }
    if (bad) Q.status[blockIdx.y] = 1;                                     // (every writer writes 1)
}

// Which of two candidates (value, free column?, position in `remaining`) the sequential scan ends on: the lower value; among equals a
// free column before a taken one, the LAST free one, the FIRST taken one.  (INFINITY, false, 0x7fffffff) loses against every position.
__device__ __forceinline__ bool lpf_as_better(double v, bool fr, int pos, double bv, bool bfr, int bpos)
{
    if (v < bv) return true;
    if (!(v == bv)) return false;
    if (fr != bfr) return fr;
    return fr ? pos > bpos : pos < bpos;
}

__global__ __launch_bounds__(64) void lpf_as_solve(const LpfAsParams Q)
{
    __shared__ double s_u[LPF_AS_CAP], s_v[LPF_AS_CAP], s_spc[LPF_AS_CAP];
    __shared__ int s_path[LPF_AS_CAP], s_row4col[LPF_AS_CAP], s_col4row[LPF_AS_CAP], s_rem[LPF_AS_CAP];
    __shared__ unsigned char s_SR[LPF_AS_CAP], s_SC[LPF_AS_CAP];
    __shared__ int s_ok;
    const LpfM2Frame fr = Q.frames[blockIdx.x];
    const int lane = threadIdx.x;
    const int D = fr.D, nl = Q.nlive[blockIdx.x];
    int *const col = Q.col + ((long long)fr.d0 - Q.col_base);
    for (int d = lane; d < D; d += 64) col[d] = -1;
    if (D <= 0 || nl <= 0 || Q.status[blockIdx.x] != 0) return;           // nothing to assign, or invalid entries
    if (D > LPF_AS_CAP || nl > LPF_AS_CAP) {                               // (refused by the host; never solved here)
        if (lane == 0) Q.status[blockIdx.x] = 2;
        return;
    }
    const bool tall = nl < D;
    const int nr = tall ? nl : D, nc = tall ? D : nl;
    const double *const S = Q.scratch + (fr.p0 - Q.scr_pair_base);        // [nr][nc]

    for (int j = lane; j < nc; j += 64) { s_v[j] = 0.0; s_row4col[j] = -1; s_path[j] = -1; }
    for (int i = lane; i < nr; i += 64) { s_u[i] = 0.0; s_col4row[i] = -1; }
    bool failed = false;
    for (int cur = 0; cur < nr && !failed; ++cur) {
        for (int j = lane; j < nc; j += 64) { s_spc[j] = INFINITY; s_SC[j] = 0; s_rem[j] = nc - 1 - j; }
        for (int i = lane; i < nr; i += 64) s_SR[i] = 0;
        __syncthreads();
        double minVal = 0.0;
        int i = cur, n_rem = nc, sink = -1;
        for (int step = 0; step < nc; ++step) {                            // a step takes one column out of `remaining`
            if (lane == 0) s_SR[i] = 1;
            const double ui = s_u[i];
            const double *const row = S + (long long)i * nc;
            double bv = INFINITY;
            bool bfr = false;
            int bpos = 0x7fffffff;
            for (int it = lane; it < n_rem; it += 64) {
                const int j = s_rem[it];
                const double r = ((minVal + row[j]) - ui) - s_v[j];
                double s = s_spc[j];
                if (r < s) { s = r; s_spc[j] = r; s_path[j] = i; }
                const bool f = s_row4col[j] == -1;
                if (lpf_as_better(s, f, it, bv, bfr, bpos)) { bv = s; bfr = f; bpos = it; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o);
                const int of = __shfl_xor((int)bfr, o), op = __shfl_xor(bpos, o);
                if (lpf_as_better(ov, of != 0, op, bv, bfr, bpos)) { bv = ov; bfr = of != 0; bpos = op; }
            }
            __syncthreads();                                               // this step's spc and path
            if (bpos < 0 || bpos >= n_rem || !(bv < INFINITY)) { failed = true; break; }     // no column can be reached
            minVal = bv;
            const int j = s_rem[bpos], last = s_rem[n_rem - 1];
            const int r4 = s_row4col[j];
            __syncthreads();                                               // (read before lane 0 rewrites the position)
            if (lane == 0) { s_SC[j] = 1; s_rem[bpos] = last; }
            --n_rem;
            if (r4 == -1) { sink = j; break; }
            if (r4 < 0 || r4 >= nr) { failed = true; break; }
            i = r4;
            __syncthreads();
        }
        if (sink < 0) failed = true;
        if (failed) break;
        __syncthreads();
        // the duals (spc of this path is read by all before the next path resets it)
        for (int k = lane; k < nr; k += 64) {
            if (k == cur) s_u[k] += minVal;
            else if (s_SR[k]) {
                const int c4 = s_col4row[k];
                if (c4 >= 0 && c4 < nc) s_u[k] += minVal - s_spc[c4];
            }
        }
        for (int j = lane; j < nc; j += 64)
            if (s_SC[j]) s_v[j] -= minVal - s_spc[j];
        __syncthreads();
        // augment along the path: sink back to cur
        if (lane == 0) {
            int j = sink;
            bool ok = false;
            for (int n = 0; n <= nr; ++n) {
                const int pi = s_path[j];
                if (pi < 0 || pi >= nr) break;
                s_row4col[j] = pi;
                const int t = s_col4row[pi];
                s_col4row[pi] = j;
                j = t;
                if (pi == cur) { ok = true; break; }
                if (j < 0 || j >= nc) break;
            }
            s_ok = ok ? 1 : 0;
        }
        __syncthreads();
        if (!s_ok) failed = true;
        __syncthreads();
    }
    if (failed) {                                                          // wave-uniform
        if (lane == 0) Q.status[blockIdx.x] = 2;
        return;
    }
    const int *const map = Q.colmap + ((long long)fr.b0 - Q.scr_box_base);
    for (int k = lane; k < nr; k += 64) {
        const int c4 = s_col4row[k];
        if (c4 < 0 || c4 >= nc) continue;
        if (tall) col[c4] = map[k];                                        // the solver's rows are the live columns
        else col[k] = map[c4];
    }
}

template <typename T>
__global__ __launch_bounds__(LPF_BLOCK) void lpf_as_finish(const LpfAsParams Q)
{
    const LpfM2Frame fr = Q.frames[blockIdx.x];
    for (int d = threadIdx.x; d < fr.D; d += LPF_BLOCK) {
        const int j = Q.col[(long long)fr.d0 + d - Q.col_base];
        double iou = 0.0, cs = 0.0, ss = 0.0, st = 0.0, tot = 0.0;
        int acc = 0;
        if (j >= 0 && j < fr.B) {
            const T *p = (const T *)Q.dets + ((long long)fr.d0 + d - Q.det_base) * 4;
            const T x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
            const T ar = (x2 - x1) * (y2 - y1);
            const T cx = (x1 + x2) / (T)2, cy = (y1 + y2) / (T)2;
            const double *q = Q.bbox2d + ((long long)fr.b0 + j - Q.box_base) * 4;
            const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            lpf_m2_pair<T, true>(x1, y1, x2, y2, ar, cx, cy, q0, q1, q2, q3, (q0 + q2) / 2.0, (q1 + q3) / 2.0, (q2 - q0) * (q3 - q1), Q.w_size,
                                 iou, cs, ss, st);
            tot = (Q.w_iou * iou + Q.w_center * cs) + st;
            acc = tot >= Q.min_score && iou >= Q.min_iou;
        }
        const long long o = (long long)fr.d0 + d - Q.score_base;
        if (Q.iou) Q.iou[o] = iou;
        if (Q.center) Q.center[o] = cs;
        if (Q.size) Q.size[o] = ss;
        if (Q.total) Q.total[o] = tot;
        if (Q.accepted) Q.accepted[o] = acc;
    }
}
