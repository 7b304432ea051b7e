// lpf_box_views.hip.h -- secondtest.py's camera-view filter and V5's detailed box projection for every box of a batch of frames
// (lpf_box_views, include/lpf.h).
//
// secondtest.py:277-419 (is_bbox_in_camera_view / filter_bboxes_in_camera_view) and V5:215-252 (project_3d_bbox_to_2d) make one
// cam2image call and a dozen small NumPy operations per box: 40 us each on the host.  This is both for F frames in one launch.
//
// The arithmetic is the reference's, statement for statement (every operation separate: the library is built with -ffp-contract=off):
//   cam2image on the raw cam-0 corners as lpf_box_prep_kernel does it: k-ordered fma chains over K, d == 0 -> -1e-6,
//   u = rint(qx / |d|), v = rint(qy / |d|) (half to even)
//   near = depth_lo <= d <= depth_hi;  n_near = its count;  in_view = near corners with 0 <= u < W and 0 <= v < H
//   verdict, in the reference's order:  n_near == 0 -> all_behind_camera (2)
//     in_view < min_points_in_view and the near corners' pixel box misses the image (x1 < 0 or x0 >= W or y1 < 0 or y0 >= H)
//       -> no_intersection (3)
//     n_near >= 2 and (umax - umin) * (vmax - vmin) < min_area -> too_small (4);  else valid (0)
//   avg_depth = np.mean(depth[near]): NumPy's summation order -- fewer than 8 values: left to right from 0.0; exactly 8:
//   ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)) -- then one division by the count
//   front = d > 0: its count, its pixel box (what lpf_box_prep_kernel writes: the sentinels +-1e300 when the set is empty) and its mean
//   depth in the same order;  corners_velo = transform_bboxes_to_velodyne as lpf_box_prep_kernel has it
//
// One launch: ONE BLOCK PER FRAME, eight lanes per box (lane = corner), LPF_BV_TILE boxes per pass of the block.  kept_pos -- a kept
// box's rank among the kept boxes of its frame, in list order -- needs an ordered prefix over the frame: a wave's kept boxes are one
// ballot, the waves' counts of a tile meet in LDS (two buffers in turn, so one barrier per tile), and the running count of the tiles
// before is carried in a register.  No atomics, no block waits for another.  The per-frame counts of each reason are wave ballots
// summed over the block at the end; a frame without boxes writes its zeros.  Only what was asked for is computed and stored.
// Corners are not validated: every address depends only on the frame table, so nothing is read or written out of bounds whatever
// they hold (non-finite corners: unspecified values).
#pragma once
#include "lpf_kernels.hip.h"

#define LPF_BV_BLOCK 512                      // 8 waves
#define LPF_BV_WAVES (LPF_BV_BLOCK / 64)
#define LPF_BV_TILE (LPF_BV_BLOCK / 8)        // boxes per pass of a block

struct LpfBvFrame { int b0, B; };             // one frame of the batch: boxes b0 .. b0 + B of the caller's arrays

struct LpfBvParams {
    const LpfBvFrame *frames;                 // the range's frames: frame blockIdx.x
    const double *corners;                    // [..][8][3]; box b of the batch at corners + (b - in_base) * 24
    int in_base, out_base;                    // first box held at corners / at the per-box outputs (0 when the caller's own arrays)
    double K[9], Tcv[16];                     // camera.K[:3,:3]; cam -> velo (read only with corners_velo)
    int W, H, min_in_view;
    double depth_lo, depth_hi, min_area;
    uint8_t *keep;                            // null: not wanted (each of the twelve)
    int *reason, *in_view, *n_near;
    double *avg_depth, *near_bbox2d;
    int *front;
    double *bbox2d, *front_avg_depth;
    int *kept_pos;
    int *frame_counts;                        // [frames of the range][6]
    double *corners_velo;
};

// np.mean of the depths d[k] with bit k of m set, in corner order (0.0 for none: the reference's `if n > 0 else 0`)
__device__ __forceinline__ double lpf_bv_mean(const double (&d)[8], unsigned m)
{
    const int n = __popc(m);
    if (n == 0) return 0.0;
    double s;
    if (n == 8) {
        s = ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]));
    } else {
        s = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if ((m >> k) & 1u) s += d[k];
    }
    return s / (double)n;
}

__global__ __launch_bounds__(LPF_BV_BLOCK) void lpf_box_views_kernel(const LpfBvParams Q)
{
    __shared__ int s_kept[2][LPF_BV_WAVES];
    __shared__ int s_why[LPF_BV_WAVES][4];
    const LpfBvFrame fr = Q.frames[blockIdx.x];
    const int tid = threadIdx.x, lane = lpf_lane(), wave = lpf_wave();
    const int k = tid & 7, sh = lane & 56;                               // corner; first lane of the box's group
    const double *K = Q.K;
    const bool want_avg = Q.avg_depth || Q.front_avg_depth;
    int running = 0;                                                     // kept boxes of the tiles before
    int why0 = 0, why2 = 0, why3 = 0, why4 = 0;                          // this wave's boxes per reason
    int par = 0;

    for (int t0 = 0; t0 < fr.B; t0 += LPF_BV_TILE) {                     // (block-uniform)
        const int j = t0 + (tid >> 3);                                   // box of the frame
        const bool live = j < fr.B;
        const long long b = (long long)fr.b0 + j;                        // box of the batch
        double x = 0, y = 0, z = 0;
        if (live) { const double *c = Q.corners + ((b - Q.in_base) * 8 + k) * 3; x = c[0]; y = c[1]; z = c[2]; }
        // cam2image on the raw cam-0 corners
        double qx = K[0] * x; qx = fma(K[1], y, qx); qx = fma(K[2], z, qx);
        double qy = K[3] * x; qy = fma(K[4], y, qy); qy = fma(K[5], z, qy);
        double d  = K[6] * x; d  = fma(K[7], y, d);  d  = fma(K[8], z, d);
        if (d == 0.0) d = -1e-6;
        const double ad = fabs(d);
        const double ru = rint(qx / ad), rv = rint(qy / ad);
        const bool in_img = (ru >= 0.0) && (ru < (double)Q.W) && (rv >= 0.0) && (rv < (double)Q.H);
        const bool near = live && (d >= Q.depth_lo) && (d <= Q.depth_hi);
        const bool fro = live && (d > 0.0);
        const unsigned near_m = (unsigned)((__ballot(near) >> sh) & 0xFFull);
        const unsigned view_m = (unsigned)((__ballot(near && in_img) >> sh) & 0xFFull);
        const unsigned front_m = (unsigned)((__ballot(fro) >> sh) & 0xFFull);
        const int n_near = __popc(near_m), n_view = __popc(view_m), n_front = __popc(front_m);
        // pixel boxes of the near and of the front corners (lanes of one box are contiguous and 8-aligned inside the wave)
        const double nx0 = lpf_min8(near ? ru : 1e300), nx1 = lpf_max8(near ? ru : -1e300);
        const double ny0 = lpf_min8(near ? rv : 1e300), ny1 = lpf_max8(near ? rv : -1e300);
        int why;
        if (n_near == 0) why = 2;
        else if (n_view < Q.min_in_view && (nx1 < 0.0 || nx0 >= (double)Q.W || ny1 < 0.0 || ny0 >= (double)Q.H)) why = 3;
        else if (n_near >= 2 && (nx1 - nx0) * (ny1 - ny0) < Q.min_area) why = 4;
        else why = 0;
        const bool lead = live && k == 0;

        // the ordered rank of the kept boxes, and the counts per reason
        const unsigned long long kept_b = __ballot(lead && why == 0);
        why0 += __popcll(kept_b);
        why2 += __popcll(__ballot(lead && why == 2));
        why3 += __popcll(__ballot(lead && why == 3));
        why4 += __popcll(__ballot(lead && why == 4));
        if (lane == 0) s_kept[par][wave] = __popcll(kept_b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < LPF_BV_WAVES; ++w) {
            const int n = s_kept[par][w];
            before += w < wave ? n : 0;
            total += n;
        }
        const int rank = running + before + __popcll(kept_b & ((1ull << lane) - 1ull));
        running += total;
        par ^= 1;

        double avg_near = 0.0, avg_front = 0.0;
        if (want_avg) {                                                  // (kernel-uniform)
            double ds[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) ds[i] = __shfl(d, sh + i);
            if (Q.avg_depth) avg_near = lpf_bv_mean(ds, near_m);
            if (Q.front_avg_depth) avg_front = lpf_bv_mean(ds, front_m);
        }
        double fx0 = 0, fx1 = 0, fy0 = 0, fy1 = 0;
        if (Q.bbox2d) {
            fx0 = lpf_min8(fro ? ru : 1e300); fx1 = lpf_max8(fro ? ru : -1e300);
            fy0 = lpf_min8(fro ? rv : 1e300); fy1 = lpf_max8(fro ? rv : -1e300);
        }
        if (live) {
            const long long o = b - Q.out_base;
            if (Q.corners_velo) {
                const double *T = Q.Tcv;
                double *cv = Q.corners_velo + (o * 8 + k) * 3;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    double a = T[4 * i] * x; a = fma(T[4 * i + 1], y, a); a = fma(T[4 * i + 2], z, a); a = fma(T[4 * i + 3], 1.0, a);
                    cv[i] = a;
                }
            }
            if (k == 0) {
                if (Q.keep) Q.keep[o] = (uint8_t)(why == 0);
                if (Q.reason) Q.reason[o] = why;
                if (Q.in_view) Q.in_view[o] = n_view;
                if (Q.n_near) Q.n_near[o] = n_near;
                if (Q.avg_depth) Q.avg_depth[o] = avg_near;
                if (Q.near_bbox2d) { double *p = Q.near_bbox2d + o * 4; p[0] = nx0; p[1] = ny0; p[2] = nx1; p[3] = ny1; }
                if (Q.front) Q.front[o] = n_front;
                if (Q.bbox2d) { double *p = Q.bbox2d + o * 4; p[0] = fx0; p[1] = fy0; p[2] = fx1; p[3] = fy1; }
                if (Q.front_avg_depth) Q.front_avg_depth[o] = avg_front;
                if (Q.kept_pos) Q.kept_pos[o] = why == 0 ? rank : -1;
            }
        }
    }

    if (!Q.frame_counts) return;
    if (lane == 0) { s_why[wave][0] = why0; s_why[wave][1] = why2; s_why[wave][2] = why3; s_why[wave][3] = why4; }
    __syncthreads();
    if (tid < 6) {                                                       // codes 1 (no_corners) and 5 (error) stay on the host
        const int col = tid == 0 ? 0 : tid - 1;                          // 0 -> 0, 2 -> 1, 3 -> 2, 4 -> 3
        int n = 0;
        if (tid == 0 || (tid >= 2 && tid <= 4))
            for (int w = 0; w < LPF_BV_WAVES; ++w) n += s_why[w][col];
        Q.frame_counts[(size_t)blockIdx.x * 6 + tid] = n;
    }
}
