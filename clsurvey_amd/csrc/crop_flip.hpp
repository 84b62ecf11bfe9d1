// One block's share of a crop + flip copy, shared by the task loaders' gather (augment.hip) and the exemplar batch assembly
// (rehearsal.hip).
#pragma once
#include "common.hpp"

constexpr int CF_BLOCK = 256;
constexpr int CF_BATCH = 4;               // accesses per thread in flight at once (loads first, then the stores)
constexpr int CF_SEG = 4096;              // output elements per block the host aims at (16 KB, as gather_tasks_kernel)

static inline int cf_rows_per_block(int tw) { return tw >= CF_SEG ? 1 : CF_SEG / tw; }   // output lines per block

// The block's destination is one contiguous run of total = nrows * tw floats at dst, its source the nrows x tw window of one
// channel plane (line pitch Ws) whose first element is src.  Lanes run along the output line, so loads are coalesced whichever
// way the line is read; a flip only reverses the lane order inside a line.  A thread divides ONCE (its first element -> line,
// column); after that it steps by the block-uniform (q, rem) = stride / tw.
// VEC: tw % 4 == 0 and dst 16-byte aligned (decided on the host): one float4 store per 4 output columns.  The source line
// start is arbitrarily aligned (any left, odd Ws), so the loads are written as dwords and promise 4-byte alignment only; read in
// ascending order and mirrored in registers, the compiler fuses four of them into one 16-byte load, which the hardware takes at
// dword alignment (measured against per-dword loads in mirrored order: 45.1 vs 48.2 us at 3 x 256^2 -> 224^2, 22.0 vs 21.2 us
// at 72^2 -> 64^2, batch 200).
// Load: how W source elements at s become floats.  cf_load_f32 reads stored floats (the text above); cf_load_u8 reads bytes and
// decodes them through the 256-entry table `lut` of the block's channel (clhip.h, byte frames).  A byte line starts at ANY
// address, so its one wide access, the dword that holds 4 output columns, is taken only behind a test of the address itself;
// byte loads otherwise.
struct cf_load_f32 {
    template <int W, typename Src>
    __device__ __forceinline__ void operator()(Src s, float (&a)[W]) const {
#pragma unroll
        for (int j = 0; j < W; ++j) a[j] = s[j];                           // ascending addresses
    }
};

struct cf_load_u8 {
    const float* lut;                                                      // [256], LDS
    template <int W, typename Src>
    __device__ __forceinline__ void operator()(Src s, float (&a)[W]) const {
        if constexpr (W == 4) {
            if ((reinterpret_cast<uintptr_t>(s) & 3u) == 0) {
                typedef const uint32_t __attribute__((address_space(1))) gu32;
                const uint32_t u = *(gu32*)s;
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = lut[(u >> (8 * j)) & 255u];
                return;
            }
        }
        uint8_t b[W];
#pragma unroll
        for (int j = 0; j < W; ++j) b[j] = s[j];
#pragma unroll
        for (int j = 0; j < W; ++j) a[j] = lut[b[j]];
    }
};

template <bool VEC, typename Src, typename Load = cf_load_f32>
__device__ __forceinline__ void cf_copy_window(Src src, int Ws, float* __restrict__ dst, unsigned total, int tw, int flip,
                                               Load load = Load()) {
    constexpr int W = VEC ? 4 : 1;                                         // output columns per access
    const int q = (CF_BLOCK * W) / tw, rem = (CF_BLOCK * W) % tw;
    int yy = (int)(threadIdx.x * W) / tw;
    int x = (int)(threadIdx.x * W) - yy * tw;
    for (unsigned e = threadIdx.x * W; e < total; e += CF_BATCH * CF_BLOCK * W) {
        float v[CF_BATCH][W];
#pragma unroll
        for (int k = 0; k < CF_BATCH; ++k) {                               // all loads in flight before the first store
            if (e + (unsigned)k * CF_BLOCK * W < total) {
                Src s = src + (size_t)yy * Ws + (flip ? tw - W - x : x);
                float a[W];
                load(s, a);                                                // ascending addresses; mirrored in registers
#pragma unroll
                for (int j = 0; j < W; ++j) v[k][j] = flip ? a[W - 1 - j] : a[j];
            }
            x += rem;
            yy += q;
            if (x >= tw) { x -= tw; ++yy; }
        }
#pragma unroll
        for (int k = 0; k < CF_BATCH; ++k) {
            const unsigned i = e + (unsigned)k * CF_BLOCK * W;
            if (i < total) {
                if constexpr (VEC) *reinterpret_cast<float4*>(dst + i) = make_float4(v[k][0], v[k][1], v[k][2], v[k][3]);
                else dst[i] = v[k][0];
            }
        }
    }
}
