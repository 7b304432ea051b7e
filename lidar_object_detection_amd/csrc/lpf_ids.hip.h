// lpf_ids.hip.h -- lpf_set_masks_ids / lpf_run_wide_ids: instance-ID maps -> the packed label image [F][H][W] (bit m = mask m) and the
// wide passes' label planes [F][LW][H][W], decoded on the GPU.  gfx950, wave64.
//
// An ID map is one image per frame, [F][H][W] elements IT (uint16_t, widened unsigned, or int32_t); mask m of frame f is the set of
// pixels whose ID equals sel[f * M + m].  A table entry LPF_ID_NONE (INT32_MIN) selects nothing, even where an int32 map holds that
// value; equal entries each get their bit.  Every compare is made on int32 values: a uint16 ID is 0 .. 65535 after widening, so an
// entry outside that range -- -1, 65536, 65536 + 5 -- equals none of them.
//
// Both kernels have the same shape.  A block belongs to ONE frame (blockIdx.x = f * nblk + b), copies that frame's table into LDS once
// -- entry t by thread t; an entry that selects nothing (LPF_ID_NONE, at or above M, outside 0 .. 65535 for a uint16 map) as 0 -- and
// leaves beside it the words `valid`, bit m = "entry m selects something", from the waves' ballots.  After the barrier every read of
// the table is the same LDS address in all 64 lanes (a broadcast, no bank conflict; four entries per 16-byte read), and a pixel's bits
// are ANDed with `valid` once: that is all LPF_ID_NONE and the bits at or above M cost.
//   A thread takes one 16-byte group of IDs -- PER = 8 uint16 or 4 int32 pixels, ONE load, each ID read once and kept in registers
// while it is compared with every entry -- and writes the group's PER label elements (per plane, for the wide form).  A frame's first
// ID need not be 16-byte aligned: the caller's pointer is aligned to its element only, and with H * W odd the frames' bases alternate.
// So per frame: head = the elements before the first 16-byte boundary (< PER), nvec = the whole groups behind it, and the rest (< PER)
// is the tail; head and tail are read and written one element per thread by the first 2 * PER threads of the frame's block 0.  The
// stores of a group are wide (up to 16 bytes) where the destination of the frame's first group is aligned for them -- the same answer
// for every group of the frame (and plane), so the branch is uniform -- and element stores otherwise.  With H * W a multiple of 16 and
// an aligned pointer there is no head, no tail, and every load and store is wide.
//
// Every element of the destination is written exactly once, zeros included, from one read of its pixel's ID: no memset in front, no
// atomics, no read of the destination, and nothing depends on the order blocks, waves or lanes run in.
//
// Bounds come from F, H, W and M alone (no input value is an index): pixel e of frame f is read at ids[f * hw + e] and written at
// label[f * hw + e] (planes[(f * LW + w) * hw + e]) for 0 <= e < hw only -- head <= hw, head + nvec * PER <= hw, a thread with
// i >= nvec does nothing -- and the table is read at sel[f * M + t] for t < M.  The host sizes the grid from hw / PER, the most
// groups a frame can have whatever its alignment (lpf_api.hip: ids_blocks).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LPF_IDS_BLOCK 256           // one group per thread: 2048 uint16 / 1024 int32 pixels per block; = the wide table's 256 entries
#define LPF_IDS_NONE INT32_MIN      // include/lpf.h: LPF_ID_NONE

// the PER IDs of a 16-byte group, widened to int32
template <typename IT> __device__ inline void lpf_ids_unpack(const uint4 v, int (&id)[16 / sizeof(IT)])
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if constexpr (sizeof(IT) == 2) {
#pragma unroll
        for (int j = 0; j < 8; ++j) id[j] = (int)((w[j >> 1] >> (16 * (j & 1))) & 0xffffu);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) id[j] = (int)w[j];
    }
}

// N consecutive elements LT from the low bits of bits[]: stores of up to 16 bytes where `wide` says p is aligned for them
template <typename LT, int N> __device__ inline void lpf_ids_store(LT *p, const uint32_t (&bits)[N], const bool wide)
{
    constexpr int A = N * (int)sizeof(LT) < 16 ? N * (int)sizeof(LT) : 16, E = A / (int)sizeof(LT);
    struct alignas(A) Chunk { LT v[E]; };
    if (wide) {
#pragma unroll
        for (int k = 0; k < N; k += E) {
            Chunk ch;
#pragma unroll
            for (int e = 0; e < E; ++e) ch.v[e] = (LT)bits[k + e];
            *(Chunk *)(p + k) = ch;
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = (LT)bits[j];
    }
}
template <typename LT, int N> __device__ inline bool lpf_ids_wide(const LT *p)
{
    return ((uintptr_t)p & (uintptr_t)((N * (int)sizeof(LT) < 16 ? N * (int)sizeof(LT) : 16) - 1)) == 0;
}

// One table entry pushed into a pixel's accumulator: acc = acc << 1 | (id == sv).  Entries are pushed from the last one down, so
// entry k ends as bit k.  For uint16 maps both values are 0 .. 65535 (lpf_ids_entry), so (id ^ sv) - 1 has bit 31 set iff they are
// equal, and v_alignbit_b32 shifts that bit in: two VALU instructions per compare, no lane mask.  The first form of this loop,
// v_cmp_eq into an SGPR pair + v_cndmask, paid the two wait states between a VALU write of an SGPR and its VALU read on every compare
// (lpf_ids_planes<uint16_t>, M = 256 at 1408 x 376: 30 us, with one LDS read per entry as with one per four).  int32 IDs span all 32
// bits, the trick does not hold, and they keep the compare
template <typename IT> __device__ inline uint32_t lpf_ids_push(const uint32_t acc, const int id, const int sv)
{
    if constexpr (sizeof(IT) == 2) return __builtin_amdgcn_alignbit(acc, (uint32_t)(id ^ sv) - 1u, 31);
    else return acc << 1 | (uint32_t)(id == sv);
}

// PER IDs against FOUR consecutive table entries k .. k + 3, read from LDS as one 16-byte broadcast and pushed last first.  The table is
// whole in LDS (entries at or above M are 0 and lose their bits to `valid`), so the last four of a table whose M is no multiple of 4
// are read like any others
template <typename IT, int PER> __device__ inline void lpf_ids_push4(const int (&id)[PER], const int4 sv, uint32_t (&acc)[PER])
{
#pragma unroll
    for (int j = 0; j < PER; ++j)
        acc[j] = lpf_ids_push<IT>(lpf_ids_push<IT>(lpf_ids_push<IT>(lpf_ids_push<IT>(acc[j], id[j], sv.w), id[j], sv.z), id[j], sv.y), id[j], sv.x);
}

// A table entry as LDS holds it, *ok = it selects something: not LPF_ID_NONE, and for a uint16 map within 0 .. 65535 -- an entry
// outside matches no ID there.  Entries that select nothing are held as 0 and lose whatever bit they produce to `valid`
template <typename IT> __device__ inline int lpf_ids_entry(const int v, bool *ok)
{
    *ok = v != LPF_IDS_NONE && (sizeof(IT) == 4 || (uint32_t)v <= 0xffffu);
    return *ok ? v : 0;
}

// a frame's split into head | nvec groups of PER | tail, from the address of its first ID
template <typename IT> __device__ inline void lpf_ids_split(const IT *src, const long long hw, long long &head, long long &nvec)
{
    constexpr int PER = 16 / (int)sizeof(IT);
    head = (long long)(((16u - (unsigned)((uintptr_t)src & 15u)) & 15u) / (unsigned)sizeof(IT));
    if (head > hw) head = hw;
    nvec = (hw - head) / PER;
}

// the narrow label image: M <= 32 masks, elements LT of 1 / 2 / 4 bytes (M <= 8 / 16 / 32)
template <typename IT, typename LT>
__global__ __launch_bounds__(LPF_IDS_BLOCK) void lpf_ids_label(const IT *__restrict__ ids, const int32_t *__restrict__ sel,
                                                                LT *__restrict__ label, const long long hw, const int M, const unsigned nblk)
{
    constexpr int PER = 16 / (int)sizeof(IT);
    __shared__ alignas(16) int32_t s_sel[32];
    __shared__ uint32_t s_valid;
    const unsigned f = blockIdx.x / nblk, b = blockIdx.x - f * nblk;
    const int t = (int)threadIdx.x;
    if (t < 64) {                                             // wave 0: the frame's table, once per block
        bool ok;
        const int v = lpf_ids_entry<IT>(t < M ? sel[(long long)f * M + t] : LPF_IDS_NONE, &ok);
        if (t < 32) s_sel[t] = v;
        const unsigned long long have = __ballot(ok);
        if (t == 0) s_valid = (uint32_t)have;
    }
    __syncthreads();
    const uint32_t valid = s_valid;
    const IT *src = ids + (long long)f * hw;
    LT *dst = label + (long long)f * hw;
    long long head, nvec;
    lpf_ids_split<IT>(src, hw, head, nvec);
    if (b == 0 && t < 2 * PER) {                              // head and tail: one element per thread
        const long long e = t < PER ? (long long)t : head + nvec * PER + (t - PER);
        if (t < PER ? e < head : e < hw) {
            const int id = (int)src[e];
            uint32_t bits = 0;
            for (int m = 0; m < M; ++m) bits |= (uint32_t)(id == s_sel[m]) << m;
            dst[e] = (LT)(bits & valid);
        }
    }
    const long long i = (long long)b * LPF_IDS_BLOCK + t;
    if (i >= nvec) return;
    const long long p = head + i * PER;
    int id[PER];
    lpf_ids_unpack<IT>(*(const uint4 *)(src + p), id);
    uint32_t bits[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) bits[j] = 0;
    for (int m = (M - 1) & ~3; m >= 0; m -= 4) lpf_ids_push4<IT, PER>(id, *(const int4 *)(s_sel + m), bits);
#pragma unroll
    for (int j = 0; j < PER; ++j) bits[j] &= valid;
    lpf_ids_store<LT, PER>(dst + p, bits, lpf_ids_wide<LT, PER>(dst + head));
}

// the wide passes' label planes: M <= 256 masks, LW = ceil(M / 32) planes of uint32_t per frame, mask m = bit m & 31 of plane m >> 5;
// the bits at or above M of the last plane are zero (their table entries are LPF_ID_NONE)
template <typename IT>
__global__ __launch_bounds__(LPF_IDS_BLOCK) void lpf_ids_planes(const IT *__restrict__ ids, const int32_t *__restrict__ sel,
                                                                 uint32_t *__restrict__ planes, const long long hw, const int M, const int LW,
                                                                 const unsigned nblk)
{
    constexpr int PER = 16 / (int)sizeof(IT);
    __shared__ alignas(16) int32_t s_sel[LPF_IDS_BLOCK];
    __shared__ uint32_t s_valid[LPF_IDS_BLOCK / 32];
    const unsigned f = blockIdx.x / nblk, b = blockIdx.x - f * nblk;
    const int t = (int)threadIdx.x;
    {                                                         // the frame's table, once per block: entry t by thread t
        bool ok;
        const int v = lpf_ids_entry<IT>(t < M ? sel[(long long)f * M + t] : LPF_IDS_NONE, &ok);
        s_sel[t] = v;
        const unsigned long long have = __ballot(ok);
        if ((t & 63) == 0) { s_valid[t >> 5] = (uint32_t)have; s_valid[(t >> 5) + 1] = (uint32_t)(have >> 32); }
    }
    __syncthreads();
    const IT *src = ids + (long long)f * hw;
    uint32_t *dst = planes + (long long)f * LW * hw;          // plane w of the frame: dst + w * hw
    long long head, nvec;
    lpf_ids_split<IT>(src, hw, head, nvec);
    if (b == 0 && t < 2 * PER) {                              // head and tail: one pixel per thread, every plane of it
        const long long e = t < PER ? (long long)t : head + nvec * PER + (t - PER);
        if (t < PER ? e < head : e < hw) {
            const int id = (int)src[e];
            for (int w = 0; w < LW; ++w) {
                const int nb = M - 32 * w < 32 ? M - 32 * w : 32;
                uint32_t bits = 0;
                for (int k = 0; k < nb; ++k) bits |= (uint32_t)(id == s_sel[32 * w + k]) << k;
                dst[(long long)w * hw + e] = bits & s_valid[w];
            }
        }
    }
    const long long i = (long long)b * LPF_IDS_BLOCK + t;
    if (i >= nvec) return;
    const long long p = head + i * PER;
    int id[PER];
    lpf_ids_unpack<IT>(*(const uint4 *)(src + p), id);
    for (int w = 0; w < LW; ++w) {
        const int nb = M - 32 * w < 32 ? M - 32 * w : 32;
        const uint32_t valid = s_valid[w];
        uint32_t bits[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) bits[j] = 0;
        for (int k = (nb - 1) & ~3; k >= 0; k -= 4) lpf_ids_push4<IT, PER>(id, *(const int4 *)(s_sel + 32 * w + k), bits);
#pragma unroll
        for (int j = 0; j < PER; ++j) bits[j] &= valid;
        uint32_t *pw = dst + (long long)w * hw;
        lpf_ids_store<uint32_t, PER>(pw + p, bits, lpf_ids_wide<uint32_t, PER>(pw + head));
    }
}
