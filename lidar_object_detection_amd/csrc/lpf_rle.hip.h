// lpf_rle.hip.h -- lpf_set_masks_rle: run-length masks -> the packed label image [F][H][W] (bit m = mask m), decoded on the GPU.
//
// The host (lpf_set_masks_rle, lpf_api.hip) checks every run before anything is queued, zeroes the label image and stages three tables:
// the caller's runs [Rtot] {start, length} (pixels of the flattened image), the caller's run_off [F*M + 1], and the table of WORK UNITS
// it emitted while it walked the runs: unit = {run, first pixel}, the pixels first .. first + LPF_RLE_CHUNK - 1 of that run (cut at the
// run's end).  The work is split by pixels, not by runs: a run may be one pixel or the whole image (530 k pixels at 1408 x 376), and
// either way a unit is at most LPF_RLE_CHUNK pixels; an empty run has no unit.
//
// One wave per unit.  The label image has elements of 1, 2 or 4 bytes (M <= 8 / 16 / 32); the wave ORs bit m into the unit's pixels
// through 32-bit atomics on the aligned words that contain them -- lane l takes words first + l, first + l + 64, ...: the atomics of one
// wave-instruction are 256 contiguous bytes.  A word at the edge of a unit gets the bit in the unit's own elements only, so neighbours in
// the word -- another run's, another mask's, the next frame's first pixels when H * W is no multiple of the word -- keep theirs.
//
// INTEGER ORs ONLY: OR is associative, commutative and idempotent, so the image is the same whatever order the hardware takes the
// units, waves and lanes in, with runs that overlap, touch, repeat or arrive shuffled, and with 32 masks on the same pixels.  Nothing is
// read back (no-return atomics), nothing is added, no float is involved: decoding twice gives identical bytes.
//
// Bounds (checked on the host, per run, in 64 bits): 0 <= start, 0 <= length, start + length <= H * W; run < Rtot and its owner
// k = f * M + m < F * M by construction of the units.  The last word of the image may reach past its last element (1- and 2-byte
// elements with an odd pixel count): label_a is reserved at F * H * W * 4 bytes for every element size, so that word lies inside the
// allocation; its bytes past the image get OR 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LPF_RLE_CHUNK 1024          // pixels per work unit: 4 / 8 / 16 wave-instructions of atomics at 1 / 2 / 4 bytes per element
#define LPF_RLE_BLOCK 256           // 4 waves = 4 units per block
#define LPF_RLE_MAX_UNITS (1u << 24)    // units of one call (1.7e10 pixels of runs: the host's table stays under 128 MB, the grid under 2^31)

struct LpfRleJob {
    const int2 *runs;               // [Rtot] {start, length}
    const int2 *units;              // [n_units] {run, first pixel}
    const long long *run_off;       // [FM + 1]
    long long hw;                   // H * W
    int n_units, M, FM;             // FM = F * M > 0
};

template <typename LT>
__global__ __launch_bounds__(LPF_RLE_BLOCK) void lpf_rle_decode(const LpfRleJob J, uint32_t *__restrict__ label)
{
    constexpr int PER = 4 / (int)sizeof(LT), EBITS = 8 * (int)sizeof(LT);      // elements per word, bits per element
    const int lane = (int)threadIdx.x & 63;
    const int u = (int)blockIdx.x * (LPF_RLE_BLOCK / 64) + ((int)threadIdx.x >> 6);
    if (u >= J.n_units) return;
    const int2 un = J.units[u];
    const int2 rn = J.runs[un.x];
    // the (frame, mask) that owns the run: the last k with run_off[k] <= run (run_off[0] = 0 <= run < run_off[FM]; empty masks repeat
    // an offset, and the last of the equal ones is the owner)
    int lo = 0, hi = J.FM;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (J.run_off[mid] <= (long long)un.x) lo = mid; else hi = mid;
    }
    const int f = lo / J.M, m = lo - f * J.M;
    const long long base = (long long)f * J.hw;
    const long long e0 = base + un.y;                                         // elements [e0, e1) of the whole [F][H][W] image
    long long e1 = base + (long long)rn.x + rn.y;
    if (e1 > e0 + LPF_RLE_CHUNK) e1 = e0 + LPF_RLE_CHUNK;
    const uint32_t bit = 1u << m;
    const long long w1 = (e1 - 1) / PER;
    for (long long w = e0 / PER + lane; w <= w1; w += 64) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const long long e = w * PER + j;
            if (e >= e0 && e < e1) v |= bit << (j * EBITS);
        }
        atomicOr(label + w, v);
    }
}

// The same runs into the wide pass's label planes [F][LW][H][W] uint32, LW = ceil(M / 32) (lpf_run_wide, lpf_run_cams_wide: wide_pack
// zeroes ALL F * LW * H * W words first, so the bits of the last word above M are zero, as the dense pack leaves them).  The same job,
// unit table and owner search; mask m of frame f lives in plane f * LW + (m >> 5) as bit m & 31.  An element is a whole word here:
// lane l ORs the bit into pixels first + l, first + l + 64, ... of the unit -- again 256 contiguous bytes per wave-instruction -- and
// no word has a neighbour to spare.  No-return integer ORs only: the planes are the same in any order, with overlap, with repeats and
// with 256 masks on one pixel (eight words, 32 ORs each).
// Bounds (the host's check, rle_walk in lpf_api.hip): f < F, m < M, so the plane is one of the F * LW that were zeroed; the unit's
// pixels are [first, min(first + LPF_RLE_CHUNK, start + length)) inside [start, start + length) inside [0, H * W).
__global__ __launch_bounds__(LPF_RLE_BLOCK) void lpf_rle_decode_wide(const LpfRleJob J, const int LW, uint32_t *__restrict__ planes)
{
    const int lane = (int)threadIdx.x & 63;
    const int u = (int)blockIdx.x * (LPF_RLE_BLOCK / 64) + ((int)threadIdx.x >> 6);
    if (u >= J.n_units) return;
    const int2 un = J.units[u];
    const int2 rn = J.runs[un.x];
    int lo = 0, hi = J.FM;                                                     // the owner, as lpf_rle_decode finds it
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (J.run_off[mid] <= (long long)un.x) lo = mid; else hi = mid;
    }
    const int f = lo / J.M, m = lo - f * J.M;
    const long long base = ((long long)f * LW + (m >> 5)) * J.hw;
    const long long e0 = base + un.y;
    long long e1 = base + (long long)rn.x + rn.y;
    if (e1 > e0 + LPF_RLE_CHUNK) e1 = e0 + LPF_RLE_CHUNK;
    const uint32_t bit = 1u << (m & 31);
    for (long long e = e0 + lane; e < e1; e += 64) atomicOr(planes + e, bit);
}
