// lpf_cams_wide.hip.h -- one scan labelled in up to LPF_MAX_CAMS (4) cameras with up to LPF_MAX_MASKS_WIDE (256) masks each, in one
// pass (lpf_run_cams_wide, include/lpf.h).
//
// A camera's run is lpf_run_wide's chain: the same intermediates in the same layout, consumed by the same device code (lpf_wide.hip.h),
// so camera c's results are bit-equal to lpf_run_wide's in camera c by construction.  What the pass shares is the read of the points
// and the launches:
//   lpf_cams_wide_project  one LPF_WIDE_CHUNK chunk per block, as lpf_wide_project: each thread loads its four float4 points from HBM
//                          ONCE, then runs lpf_wide_project's per-point work (lpf_wide_project_chunk, preloaded points) for every camera
//                          in turn.  The chunking depends on the points only: every camera's frame table has the same chunk fields.
//   lpf_cams_wide_scan     grid (frames, cameras)
//   lpf_cams_wide_scatter  grid (chunks, cameras)
//   lpf_cams_wide_lists    grid (frames x the most label words of any camera, cameras)
//   lpf_cams_wide_boxes    grid (the most (frame, word, 64-box word) blocks of any camera, LPF_WIDE_PARTS, cameras)
//   lpf_cams_wide_best     grid (frames, cameras)
// A block beyond its own camera's extent returns at once.  The camera records travel by value: C x sizeof(LpfWideParams) = 4 x 464
// bytes of the 4 KB of kernel arguments.  Every access to them is indexed by a wave-uniform camera (blockIdx.y / blockIdx.z, or the loop
// counter), so they stay scalar loads from the argument segment -- no table upload, no dependent global load before the first point.
// Each camera's masks are packed by lpf_wide_pack / lpf_erode_packed into planes of its own, and its box tables are built by
// lpf_box_job_kernel into lpf_run_cams' per-camera box sets.
#pragma once
#include "lpf_wide.hip.h"
#include "lpf_cams.hip.h"

struct LpfCamsWideArgs {
    LpfWideParams P[LPF_MAX_CAMS_DEV]; // camera c's lpf_run_wide chain; P[0]'s frame table also gives the pass's chunks
    int C;                             // cameras
};
static_assert(sizeof(LpfCamsWideArgs) <= 4096, "a kernel's argument segment holds 4 KB");

__global__ __launch_bounds__(LPF_BLOCK) void lpf_cams_wide_project(const LpfCamsWideArgs A)
{
    __shared__ unsigned s_tmp[8];
    const int c = blockIdx.x;
    const int f = lpf_wide_frame_of_chunk(A.P[0], c);
    const LpfWideFrame fr = A.P[0].frames[f];
    const int base = (c - fr.chunk_off) * LPF_WIDE_CHUNK;
    float4 p[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = base + threadIdx.x * 4 + r;
        p[r] = i < fr.N ? A.P[0].pts[(size_t)fr.pt_off + i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int cam = 0; cam < A.C; ++cam)                    // (uniform)
        lpf_wide_project_chunk<true>(A.P[cam], c, f, fr, p, s_tmp);
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_cams_wide_scan(const LpfCamsWideArgs A)
{
    __shared__ unsigned s_tmp[8];
    lpf_wide_scan_frame(A.P[blockIdx.y], blockIdx.x, s_tmp);
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_cams_wide_scatter(const LpfCamsWideArgs A)
{
    __shared__ unsigned s_tmp[8];
    lpf_wide_scatter_chunk(A.P[blockIdx.y], blockIdx.x, s_tmp);
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_cams_wide_lists(const LpfCamsWideArgs A)
{
    __shared__ unsigned s_cnt[32], s_run[32], s_wc[4][32], s_before;
    const LpfWideParams &W = A.P[blockIdx.y];
    if ((int)blockIdx.x >= W.F * max(W.LW, 1)) return;
    lpf_wide_lists_block(W, blockIdx.x, s_cnt, s_run, s_wc, s_before);
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_cams_wide_boxes(const LpfCamsWideArgs A)
{
    __shared__ double s_bp[64 * 16];
    __shared__ float s_bq[64 * 6];
    __shared__ unsigned s_c[32 * 64];
    const LpfWideParams &W = A.P[blockIdx.z];
    if (W.M == 0 || (int)blockIdx.x >= W.F * W.LW * W.nbw) return;
    lpf_wide_boxes_block(W, blockIdx.x, blockIdx.y, s_bp, s_bq, s_c);
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_cams_wide_best(const LpfCamsWideArgs A)
{
    const LpfWideParams &W = A.P[blockIdx.y];
    if (W.M == 0) return;
    lpf_wide_best_frame(W, blockIdx.x);
}
