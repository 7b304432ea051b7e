// lpf_depth_overlays.hip.h -- per-car depth overlay images of a batch of frames (lpf_depth_overlays, include/lpf.h).
//
// seg_with_pointcloud.py:174-180, once per car with a nonzero depth map:
//   depthImage = cm(depthMap / np.max(depthMap))[..., :3];  image_withseg = masking_image / 255.
//   image_withseg[depthMap > 0] = depthImage[depthMap > 0];  np.uint8(image_withseg * 255);  cvtColor(RGB2BGR)
// Byte for byte that is: every pixel the channel-reversed segmented pixel, except the car's listed pixels, which get the reversed
// jet colour lpf_jet_u8[min(255, (int)(256.0 * (d / mx)))] (matplotlib's Colormap.__call__ on floats; mx the car's np.max).
// Two launches in stream order over a chunk of (frame, car) images; no block waits for another:
//   lpf_do_render   one thread per group of P pixels (P = 16: three dwordx4 loads and stores; P = 4: three dwords; P = 1: bytes) of
//                   one image: the frame's segmented pixels with their bytes reversed in registers
//   lpf_do_paint    one wave per (frame, car): the fp64 max of the car's depths (exact and order-free), written to max_depth, then
//                   lane per list entry the jet colour of that pixel (behind the render of the same image in stream order)
// The lists come from lpf_depth_maps and are not checked when they live on the device: the offsets are clamped to [0, cap] and
// non-decreasing, pixels outside [0, W * H) are skipped, colour indices are clamped to [0, 255].
#pragma once
#include "lpf_kernels.hip.h"

// (cm._lut[:256, :3] * 255).astype(np.uint8) of matplotlib's 'jet' (matplotlib 3.10; tests/golden/jet_lut_u8.npy holds the same table)
__constant__ unsigned char lpf_jet_u8[256][3] = {
    {0, 0, 127}, {0, 0, 132}, {0, 0, 136}, {0, 0, 141}, {0, 0, 145}, {0, 0, 150}, {0, 0, 154}, {0, 0, 159},
    {0, 0, 163}, {0, 0, 168}, {0, 0, 172}, {0, 0, 177}, {0, 0, 182}, {0, 0, 186}, {0, 0, 191}, {0, 0, 195},
    {0, 0, 200}, {0, 0, 204}, {0, 0, 209}, {0, 0, 213}, {0, 0, 218}, {0, 0, 222}, {0, 0, 227}, {0, 0, 232},
    {0, 0, 236}, {0, 0, 241}, {0, 0, 245}, {0, 0, 250}, {0, 0, 254}, {0, 0, 255}, {0, 0, 255}, {0, 0, 255},
    {0, 0, 255}, {0, 4, 255}, {0, 8, 255}, {0, 12, 255}, {0, 16, 255}, {0, 20, 255}, {0, 24, 255}, {0, 28, 255},
    {0, 32, 255}, {0, 36, 255}, {0, 40, 255}, {0, 44, 255}, {0, 48, 255}, {0, 52, 255}, {0, 56, 255}, {0, 60, 255},
    {0, 64, 255}, {0, 68, 255}, {0, 72, 255}, {0, 76, 255}, {0, 80, 255}, {0, 84, 255}, {0, 88, 255}, {0, 92, 255},
    {0, 96, 255}, {0, 100, 255}, {0, 104, 255}, {0, 108, 255}, {0, 112, 255}, {0, 116, 255}, {0, 120, 255}, {0, 124, 255},
    {0, 128, 255}, {0, 132, 255}, {0, 136, 255}, {0, 140, 255}, {0, 144, 255}, {0, 148, 255}, {0, 152, 255}, {0, 156, 255},
    {0, 160, 255}, {0, 164, 255}, {0, 168, 255}, {0, 172, 255}, {0, 176, 255}, {0, 180, 255}, {0, 184, 255}, {0, 188, 255},
    {0, 192, 255}, {0, 196, 255}, {0, 200, 255}, {0, 204, 255}, {0, 208, 255}, {0, 212, 255}, {0, 216, 255}, {0, 220, 254},
    {0, 224, 250}, {0, 228, 247}, {2, 232, 244}, {5, 236, 241}, {8, 240, 237}, {12, 244, 234}, {15, 248, 231}, {18, 252, 228},
    {21, 255, 225}, {24, 255, 221}, {28, 255, 218}, {31, 255, 215}, {34, 255, 212}, {37, 255, 208}, {41, 255, 205}, {44, 255, 202},
    {47, 255, 199}, {50, 255, 195}, {54, 255, 192}, {57, 255, 189}, {60, 255, 186}, {63, 255, 183}, {66, 255, 179}, {70, 255, 176},
    {73, 255, 173}, {76, 255, 170}, {79, 255, 166}, {83, 255, 163}, {86, 255, 160}, {89, 255, 157}, {92, 255, 154}, {95, 255, 150},
    {99, 255, 147}, {102, 255, 144}, {105, 255, 141}, {108, 255, 137}, {112, 255, 134}, {115, 255, 131}, {118, 255, 128}, {121, 255, 125},
    {124, 255, 121}, {128, 255, 118}, {131, 255, 115}, {134, 255, 112}, {137, 255, 108}, {141, 255, 105}, {144, 255, 102}, {147, 255, 99},
    {150, 255, 95}, {154, 255, 92}, {157, 255, 89}, {160, 255, 86}, {163, 255, 83}, {166, 255, 79}, {170, 255, 76}, {173, 255, 73},
    {176, 255, 70}, {179, 255, 66}, {183, 255, 63}, {186, 255, 60}, {189, 255, 57}, {192, 255, 54}, {195, 255, 50}, {199, 255, 47},
    {202, 255, 44}, {205, 255, 41}, {208, 255, 37}, {212, 255, 34}, {215, 255, 31}, {218, 255, 28}, {221, 255, 24}, {224, 255, 21},
    {228, 255, 18}, {231, 255, 15}, {234, 255, 12}, {237, 255, 8}, {241, 252, 5}, {244, 248, 2}, {247, 244, 0}, {250, 240, 0},
    {254, 237, 0}, {255, 233, 0}, {255, 229, 0}, {255, 226, 0}, {255, 222, 0}, {255, 218, 0}, {255, 215, 0}, {255, 211, 0},
    {255, 207, 0}, {255, 203, 0}, {255, 200, 0}, {255, 196, 0}, {255, 192, 0}, {255, 189, 0}, {255, 185, 0}, {255, 181, 0},
    {255, 177, 0}, {255, 174, 0}, {255, 170, 0}, {255, 166, 0}, {255, 163, 0}, {255, 159, 0}, {255, 155, 0}, {255, 152, 0},
    {255, 148, 0}, {255, 144, 0}, {255, 140, 0}, {255, 137, 0}, {255, 133, 0}, {255, 129, 0}, {255, 126, 0}, {255, 122, 0},
    {255, 118, 0}, {255, 115, 0}, {255, 111, 0}, {255, 107, 0}, {255, 103, 0}, {255, 100, 0}, {255, 96, 0}, {255, 92, 0},
    {255, 89, 0}, {255, 85, 0}, {255, 81, 0}, {255, 77, 0}, {255, 74, 0}, {255, 70, 0}, {255, 66, 0}, {255, 63, 0},
    {255, 59, 0}, {255, 55, 0}, {255, 52, 0}, {255, 48, 0}, {255, 44, 0}, {255, 40, 0}, {255, 37, 0}, {255, 33, 0},
    {255, 29, 0}, {255, 26, 0}, {255, 22, 0}, {254, 18, 0}, {250, 15, 0}, {245, 11, 0}, {241, 7, 0}, {236, 3, 0},
    {232, 0, 0}, {227, 0, 0}, {222, 0, 0}, {218, 0, 0}, {213, 0, 0}, {209, 0, 0}, {204, 0, 0}, {200, 0, 0},
    {195, 0, 0}, {191, 0, 0}, {186, 0, 0}, {182, 0, 0}, {177, 0, 0}, {172, 0, 0}, {168, 0, 0}, {163, 0, 0},
    {159, 0, 0}, {154, 0, 0}, {150, 0, 0}, {145, 0, 0}, {141, 0, 0}, {136, 0, 0}, {132, 0, 0}, {127, 0, 0},
};

struct LpfDoParams {
    long long hw;                           // W * H pixels per image
    long long i0, n;                        // the chunk: images i0 .. i0 + n of the batch, image i = frame i / M, car i % M
    int M;
    long long cap;
    long long seg_f0, list_f0;              // first frame held at seg / at pix, depth and car_off (0 when the caller's own arrays)
    const unsigned char *seg;               // [..][H][W][3]
    const long long *pix;                   // [..][cap]
    const double *depth;                    // [..][cap]
    const long long *car_off;               // [..][M + 1]
    unsigned char *img;                     // image i0 + k at img + k * hw * 3 (null: no images)
    double *mx;                             // [F][M] np.max of car (frame, m) at mx[frame * M + m] (null: not wanted)
};

// the 3 * P / 4 dwords of P pixels, each pixel's three bytes reversed (byte o of the group comes from byte 3 (o / 3) + 2 - o % 3)
template <int P>
__device__ __forceinline__ void lpf_do_swap(const uint32_t *w, uint32_t *o)
{
#pragma unroll
    for (int j = 0; j < 3 * P / 4; ++j) {
        uint32_t r = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int ob = 4 * j + b, sb = 3 * (ob / 3) + 2 - ob % 3;
            r |= ((w[sb >> 2] >> (8 * (sb & 3))) & 0xffu) << (8 * b);
        }
        o[j] = r;
    }
}

template <int P>
__global__ __launch_bounds__(LPF_BLOCK) void lpf_do_render(const LpfDoParams Q)
{
    const long long k = blockIdx.y;                                         // image of the chunk
    const long long i = Q.i0 + k, f = i / Q.M;
    const long long g = (long long)blockIdx.x * LPF_BLOCK + threadIdx.x;   // pixel group
    const long long p0 = g * P;
    if (p0 >= Q.hw) return;
    const unsigned char *__restrict__ s = Q.seg + (f - Q.seg_f0) * Q.hw * 3 + p0 * 3;
    unsigned char *__restrict__ d = Q.img + k * Q.hw * 3 + p0 * 3;
    if constexpr (P > 1) {
        if (p0 + P <= Q.hw) {                       // (the host picks P so that P divides W * H and the bases are aligned to 4 P)
            uint32_t w[3 * P / 4], o[3 * P / 4];
            if (P == 16) {
                const uint4 *sv = (const uint4 *)s;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const uint4 v = sv[q];
                    w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 3 * P / 4; ++q) w[q] = ((const uint32_t *)s)[q];
            }
            lpf_do_swap<P>(w, o);
            if (P == 16) {
                uint4 *dv = (uint4 *)d;
#pragma unroll
                for (int q = 0; q < 3; ++q) dv[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
            } else {
#pragma unroll
                for (int q = 0; q < 3 * P / 4; ++q) ((uint32_t *)d)[q] = o[q];
            }
            return;
        }
    }
    for (long long p = 0; p < P && p0 + p < Q.hw; ++p) {                    // P = 1, or a group cut by the end of the image
        const unsigned char a = s[3 * p], b = s[3 * p + 1], c = s[3 * p + 2];
        d[3 * p] = c; d[3 * p + 1] = b; d[3 * p + 2] = a;
    }
}

__global__ __launch_bounds__(LPF_BLOCK) void lpf_do_paint(const LpfDoParams Q)
{
    const long long k = (long long)blockIdx.x * 4 + lpf_wave();
    if (k >= Q.n) return;
    const int lane = lpf_lane();
    const long long i = Q.i0 + k, f = i / Q.M;
    const int m = (int)(i - f * Q.M);
    const long long *off = Q.car_off + (f - Q.list_f0) * (Q.M + 1);
    const long long a = min(max(off[m], 0ll), Q.cap);
    const long long b = max(min(max(off[m + 1], 0ll), Q.cap), a);
    const long long row = (f - Q.list_f0) * Q.cap;
    double mx = 0.0;
    for (long long e = a + lane; e < b; e += 64) mx = fmax(mx, Q.depth[row + e]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (Q.mx && lane == 0) Q.mx[i] = mx;
    if (!Q.img) return;
    unsigned char *__restrict__ d = Q.img + k * Q.hw * 3;
    for (long long e = a + lane; e < b; e += 64) {
        const long long p = Q.pix[row + e];
        if (p < 0 || p >= Q.hw) continue;
        const double x = 256.0 * (Q.depth[row + e] / mx);                  // one IEEE division; * 256 is exact
        const int c = (int)fmin(fmax(x, 0.0), 255.0);                       // = min(255, (int)x) for x in [0, 256]; NaN -> 0
        d[3 * p] = lpf_jet_u8[c][2];
        d[3 * p + 1] = lpf_jet_u8[c][1];
        d[3 * p + 2] = lpf_jet_u8[c][0];
    }
}
