// lpf_cams.hip.h -- one scan labelled in up to LPF_MAX_CAMS (4) cameras in one pass (lpf_run_cams, include/lpf.h).
//
// A camera's run is the narrow in-order run: the same intermediates in the same layout, consumed by the same device code.  What the
// pass shares is the stream over the points and the launches:
//   lpf_cams_stream    one K1 tile per block, as lpf_k1_project_t: lpf_k1_tile with camera 0's LpfParams loads the tile's float4
//                      points from HBM ONCE and does its work; the other cameras' calls reuse the points in registers (PRELOADED).  Each
//                      call runs the tile's per-row work in that camera's arithmetic -- transform, rounding, clip, label gather, ballots,
//                      hand-off list, counters -- into camera c's scratch set.  The tile geometry (segments, the frame records' point
//                      fields) depends on the points only: every camera's call finds the same tile.
//   lpf_cams_tail      lists and box counts: grid (blocks of the camera with the most, cameras); a block past its camera's count
//                      leaves at once, the others are lpf_tail_t's blocks (lpf_tail_block).
//   lpf_cams_finalize  grid (frames, cameras): lpf_finalize_frame of camera c.
// The camera records travel by value: C x sizeof(LpfParams) = 4 x 576 bytes of the 4 KB of kernel arguments.  Every access to them
// is indexed by a wave-uniform camera (blockIdx.y, or the loop counter), so they stay scalar loads from the argument segment.
// Each camera's masks are packed by the narrow path's own pack kernels (lpf_pack16 / lpf_pack_erode / lpf_erode_packed) into label
// images of ONE element type for the pass, and its box tables are built by lpf_box_job_kernel.
#pragma once
#include "lpf_kernels.hip.h"

#define LPF_MAX_CAMS_DEV 4             // = LPF_MAX_CAMS of include/lpf.h = LPF_NSETS of lpf_api.hip (a scratch set per camera)

struct LpfCamsArgs {
    LpfParams P[LPF_MAX_CAMS_DEV];     // camera c's run; P[0] also gives the pass's tile geometry
    int C;                             // cameras
    int ntail[LPF_MAX_CAMS_DEV];       // tail blocks of camera c (count blocks first, then list blocks: lpf_tail_block)
};
static_assert(sizeof(LpfCamsArgs) <= 4096, "a kernel's argument segment holds 4 KB");

template <int ROWS, typename LT>
__global__ __launch_bounds__(LPF_BLOCK) void lpf_cams_stream(const LpfCamsArgs A)
{
    __shared__ unsigned s_cnt[LPF_MAX_CAMS_DEV][LPF_TAB_ROWS];      // a counter row per camera: camera c + 1 may clear its own while
                                                                    // camera c's are still being read
    float4 p[ROWS];
    lpf_k1_tile<ROWS, LPF_K1_FLAGS, LT, false>(A.P[0], (int)blockIdx.x, s_cnt[0], p);     // loads the tile's points
    for (int cam = 1; cam < A.C; ++cam)                                                    // (uniform)
        lpf_k1_tile<ROWS, LPF_K1_FLAGS, LT, true>(A.P[cam], (int)blockIdx.x, s_cnt[cam], p);
}

template <bool PRE>
__global__ __launch_bounds__(LPF_BLOCK, 7) void lpf_cams_tail(const LpfCamsArgs A)
{
    __shared__ __attribute__((aligned(16))) char s_raw[LPF_TAIL_LDS];
    const int cam = (int)blockIdx.y;
    if ((int)blockIdx.x >= A.ntail[cam]) return;
    lpf_tail_block<PRE, 1>(A.P[cam], (int)blockIdx.x, s_raw);
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_cams_finalize(const LpfCamsArgs A)
{
    __shared__ unsigned s_tot[LPF_TAB_ROWS], s_c[LPF_FIN_STAGE];
    const LpfParams &P = A.P[blockIdx.y];
    const int f = (int)blockIdx.x;
    const LpfFrame fr = lpf_frame_record(P.frame0, P.frames, P.F > 1, f);
    lpf_finalize_frame(P, fr, f, s_tot, s_c);
}
