// lpf_match2d.hip.h -- V4 / V5 scoring of every (detection, projected box) pair of a batch of frames (lpf_match_2d, include/lpf.h).
//
// V4:118-183 (match_detections_to_bboxes) takes, per detection, the first strict maximum of calculate_iou_2d over the frame's projected
// boxes; V5:277-356 (calculate_matching_score) fills a cost matrix 1 - (w_iou iou + w_center centre proximity + w_size area ratio) for
// scipy's linear_sum_assignment.  Both are double loops of Python scalars; this is the pair stage of both for F frames in one launch.
//
// The arithmetic is the reference's, type for type.  The detector's boxes are float32 and iterating them gives np.float32 scalars; a
// projected box holds np.int64 pixels (here: the same values as float64), and NumPy 2 promotes float32 (op) int64 / float64 to float64
// but keeps float32 (op) float32.  Python's max(a, b) / min(a, b) return b only when it is strictly greater / smaller, so the TYPE of an
// intersection edge depends on where it came from.  With T the detection's type (float, or double under dets_f64):
//   xa = box x0 if box x0 > det x1 else det x1;  xb = box x1 if box x1 < det x2 else det x2;  same for y;  empty if xb <= xa or yb <= ya
//   xb - xa is a T subtraction when both ends are the detection's, else float64;  inter is a T product only when both differences are T
//   area1 = (x2 - x1) * (y2 - y1) in T;  area2 in float64;  union = area1 + area2 - inter (float64, left to right)
//   iou = inter / union if union > 0 else 0
//   centre of the detection in T, of the box in float64;  dist = sqrt(fma(dy, dy, dx * dx)) (np.linalg.norm's BLAS dot);
//   center_score = c if c > 0 else 0, c = 1 - dist / 1000;  size_score = min(area1, area2) / max(area1, area2) if both > 0 else 0
//   total = w_iou * iou + w_center * center_score + w_size * size_score (left to right);  cost = 1 - total
//   equal areas: min and max both return the detection's area1, so the ratio is a T 1.0 and the Python float w_size times it is a T
//   product (Python floats are weak under NumPy 2 promotion): the size term is then (T)w_size, not w_size
// Every operation is separate (the library is built with -ffp-contract=off); `/` and sqrt are IEEE float64.
//
// One launch: grid (row groups, frames).  A block owns LPF_M2_ROWS consecutive detections of one frame, a wave LPF_M2_ROWS / 4 of
// them; the frame's boxes -- rectangle, centre, area, front -- go through LDS in tiles of LPF_M2_TILE, loaded once per block.  Lanes
// stride over the columns of a row, so a wave stores 512 contiguous bytes per matrix, and a row's V4 result is one wave reduction:
// maximum IoU, lowest column among equals (each lane meets its columns in ascending order and only a strictly greater IoU replaces
// its best, so that is the first strict maximum of the reference's scan).  Only the matrices that were asked for are computed and
// stored.  A column whose box has front == 0 is written as iou 0, scores 0, cost 1 and never wins.  Nothing is read or written outside
// the frame's rows and columns whatever the coordinates hold.
#pragma once
#include "lpf_kernels.hip.h"

#define LPF_M2_ROWS 16            // detections per block: 4 per wave
#define LPF_M2_TILE 512           // boxes per LDS tile: 7 doubles + 1 int each = 30 KB

struct LpfM2Frame {               // one frame of the batch (absolute positions in the caller's arrays)
    int d0, D;                    // detections d0 .. d0 + D
    int b0, B;                    // boxes b0 .. b0 + B
    long long p0;                 // first pair of the frame's [D][B] block
};

struct LpfM2Params {
    const LpfM2Frame *frames;     // the chunk's frames: frame blockIdx.y
    const void *dets;             // [..][4] float or double; row d of the batch at dets + (d - det_base) * 4
    const double *bbox2d;         // [..][4]; box b at bbox2d + (b - box_base) * 4
    const int *front;             // [..]
    int det_base, box_base;       // first detection / box held at dets / bbox2d (0 when the caller's own arrays)
    int det_out_base;             // first detection held at best_box / best_iou
    long long pair_base;          // first pair held at the matrices
    int *best_box;                // null: not wanted (each of the seven)
    double *best_iou;
    double *iou, *center, *size, *total, *cost;
    double min_iou, w_iou, w_center, w_size;
};

// One pair.  SCORES: the two other V5 terms beside the IoU, and the size term of the total.
template <typename T, bool SCORES>
__device__ __forceinline__ void lpf_m2_pair(T x1, T y1, T x2, T y2, T area1, T cdx, T cdy, double bx0, double by0, double bx1, double by1,
                                            double bcx, double bcy, double area2, double w_size, double &iou, double &cs, double &ss,
                                            double &st)
{
    const bool xa_box = bx0 > (double)x1, xb_box = bx1 < (double)x2;
    const bool ya_box = by0 > (double)y1, yb_box = by1 < (double)y2;
    const double xa = xa_box ? bx0 : (double)x1, xb = xb_box ? bx1 : (double)x2;
    const double ya = ya_box ? by0 : (double)y1, yb = yb_box ? by1 : (double)y2;
    iou = 0.0;
    if (!(xb <= xa || yb <= ya)) {
        const bool wt = !xa_box && !xb_box, ht = !ya_box && !yb_box;       // both ends the detection's: the difference stays in T
        const T wT = x2 - x1, hT = y2 - y1;
        const double w = wt ? (double)wT : xb - xa, h = ht ? (double)hT : yb - ya;
        const double inter = (wt && ht) ? (double)(T)(wT * hT) : w * h;
        const double uni = ((double)area1 + area2) - inter;
        if (uni > 0.0) iou = inter / uni;
    }
    if (SCORES) {
        const double dx = (double)cdx - bcx, dy = (double)cdy - bcy;
        const double c = 1.0 - sqrt(fma(dy, dy, dx * dx)) / 1000.0;
        cs = c > 0.0 ? c : 0.0;
        const double a1 = (double)area1;
        const double lo = area2 < a1 ? area2 : a1, hi = area2 > a1 ? area2 : a1;
        ss = (a1 > 0.0 && area2 > 0.0) ? lo / hi : 0.0;
        st = (a1 > 0.0 && area2 == a1) ? (double)((T)w_size * (T)1) : w_size * ss;      // the size term of the total
    }
}

template <typename T, bool SCORES>
__global__ __launch_bounds__(LPF_BLOCK) void lpf_m2_pairs(const LpfM2Params Q)
{
    __shared__ double s_x0[LPF_M2_TILE], s_y0[LPF_M2_TILE], s_x1[LPF_M2_TILE], s_y1[LPF_M2_TILE];
    __shared__ double s_cx[LPF_M2_TILE], s_cy[LPF_M2_TILE], s_ar[LPF_M2_TILE];
    __shared__ int s_fr[LPF_M2_TILE];
    constexpr int RPW = LPF_M2_ROWS / 4;
    const LpfM2Frame fr = Q.frames[blockIdx.y];
    const long long row0 = (long long)blockIdx.x * LPF_M2_ROWS;
    if (row0 >= fr.D) return;                                              // (the whole block: the grid is sized by the largest frame)
    const int tid = threadIdx.x, lane = lpf_lane(), wave = lpf_wave();
    const int B = fr.B;

    // this wave's rows: row0 + wave * RPW + r
    T x1[RPW], y1[RPW], x2[RPW], y2[RPW], ar[RPW], cx[RPW], cy[RPW];
    double best[RPW];
    int bcol[RPW];
    bool live[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const long long d = row0 + wave * RPW + r;
        live[r] = d < fr.D;
        best[r] = 0.0; bcol[r] = 0x7fffffff;
        x1[r] = y1[r] = x2[r] = y2[r] = ar[r] = cx[r] = cy[r] = (T)0;
        if (live[r]) {
            const T *p = (const T *)Q.dets + ((long long)fr.d0 + d - Q.det_base) * 4;
            x1[r] = p[0]; y1[r] = p[1]; x2[r] = p[2]; y2[r] = p[3];
            ar[r] = (x2[r] - x1[r]) * (y2[r] - y1[r]);
            cx[r] = (x1[r] + x2[r]) / (T)2; cy[r] = (y1[r] + y2[r]) / (T)2;
        }
    }

    for (int t0 = 0; t0 < B; t0 += LPF_M2_TILE) {
        const int n = min(LPF_M2_TILE, B - t0);
        __syncthreads();                                                   // the previous tile has been read
        for (int j = tid; j < n; j += LPF_BLOCK) {
            const long long b = (long long)fr.b0 + t0 + j - Q.box_base;
            const double *q = Q.bbox2d + b * 4;
            const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            s_x0[j] = q0; s_y0[j] = q1; s_x1[j] = q2; s_y1[j] = q3;
            s_cx[j] = (q0 + q2) / 2.0; s_cy[j] = (q1 + q3) / 2.0;
            s_ar[j] = (q2 - q0) * (q3 - q1);
            s_fr[j] = Q.front[b];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            if (!live[r]) continue;                                        // wave-uniform
            const long long d = row0 + wave * RPW + r;
            const long long base = fr.p0 + d * B + t0 - Q.pair_base;
            for (int j = lane; j < n; j += 64) {
                double iou = 0.0, cs = 0.0, ss = 0.0, st = 0.0, tot = 0.0, cost = 1.0;
                if (s_fr[j] > 0) {
                    lpf_m2_pair<T, SCORES>(x1[r], y1[r], x2[r], y2[r], ar[r], cx[r], cy[r], s_x0[j], s_y0[j], s_x1[j], s_y1[j],
                                           s_cx[j], s_cy[j], s_ar[j], Q.w_size, iou, cs, ss, st);
                    if (SCORES) {
                        tot = (Q.w_iou * iou + Q.w_center * cs) + st;
                        cost = 1.0 - tot;
                    }
                    if (iou > best[r]) { best[r] = iou; bcol[r] = t0 + j; }
                }
                if (Q.iou) Q.iou[base + j] = iou;
                if (SCORES) {
                    if (Q.center) Q.center[base + j] = cs;
                    if (Q.size) Q.size[base + j] = ss;
                    if (Q.total) Q.total[base + j] = tot;
                    if (Q.cost) Q.cost[base + j] = cost;
                }
            }
        }
    }

    if (!Q.best_box && !Q.best_iou) return;
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        if (!live[r]) continue;
        double v = best[r];
        int c = bcol[r];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                                 // maximum IoU, lowest column among equals
            const double ov = __shfl_xor(v, o);
            const int oc = __shfl_xor(c, o);
            if (ov > v || (ov == v && oc < c)) { v = ov; c = oc; }
        }
        if (lane == 0) {
            const bool won = v > 0.0 && v > Q.min_iou;                     // V4:176 `iou > best_iou and iou > min_iou`, best_iou from 0
            const long long d = (long long)fr.d0 + row0 + wave * RPW + r - Q.det_out_base;
            if (Q.best_box) Q.best_box[d] = won ? c : -1;
            if (Q.best_iou) Q.best_iou[d] = won ? v : 0.0;
        }
    }
}
