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
    // The two-step form (cf_copy_window_pad): fetch / fetch_one only ISSUE loads into a raw group of W elements, set_fill marks
    // an element as the fill, value() turns a raw element into its float afterwards.
    template <int W> struct raw { float v[W]; };
    template <int W, typename Src>
    __device__ __forceinline__ void fetch(Src s, raw<W>& r) const {
#pragma unroll
        for (int j = 0; j < W; ++j) r.v[j] = s[j];                         // ascending addresses
    }
    template <int W> __device__ __forceinline__ void begin_singles(raw<W>&) const {}
    template <int W, typename Src> __device__ __forceinline__ void fetch_one(Src s, raw<W>& r, int j) const { r.v[j] = s[0]; }
    template <int W> __device__ __forceinline__ void set_fill(raw<W>& r, int j, float fill) const { r.v[j] = fill; }
    template <int W> __device__ __forceinline__ float value(const raw<W>& r, int j, float) const { return r.v[j]; }
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
    // The two-step form, as cf_load_f32's: a raw element is the undecoded byte (256: the fill), or the group's dword when its
    // address was tested (packed); the table is read in value(), after the loads of a batch were issued.  A caller that marks
    // elements as fill gives `lut` 257 entries, the last one the fill: value() then needs no compare for them.
    template <int W> struct raw { uint32_t v[W]; bool packed; };
    template <int W, typename Src>
    __device__ __forceinline__ void fetch(Src s, raw<W>& r) const {
        if constexpr (W == 4) {
            if ((reinterpret_cast<uintptr_t>(s) & 3u) == 0) {
                typedef const uint32_t __attribute__((address_space(1))) gu32;
                r.v[0] = *(gu32*)s;
                r.v[1] = r.v[2] = r.v[3] = 0;
                r.packed = true;
                return;
            }
        }
        r.packed = false;
#pragma unroll
        for (int j = 0; j < W; ++j) r.v[j] = s[j];
    }
    template <int W> __device__ __forceinline__ void begin_singles(raw<W>& r) const { r.packed = false; }
    template <int W, typename Src> __device__ __forceinline__ void fetch_one(Src s, raw<W>& r, int j) const { r.v[j] = s[0]; }
    template <int W> __device__ __forceinline__ void set_fill(raw<W>& r, int j, float) const { r.v[j] = 256u; }
    template <int W> __device__ __forceinline__ float value(const raw<W>& r, int j, float) const {
        return lut[r.packed ? (r.v[0] >> (8 * j)) & 255u : r.v[j]];        // (r.v[j] <= 256)
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

// ------------------------------------------------------------------------------------------------ padded window
// torchvision's pad(padding, fill, padding_mode) of an n-long axis, as an index map: where the padded image's coordinate s
// (unpadded origin, so s < 0 is left / top padding) is taken from.  -1: nowhere, the element is the fill.  MODE is a template
// argument: the map of an interior coordinate is two compares, and no lane branches on the mode.
constexpr int CF_PAD_CONSTANT = 0, CF_PAD_EDGE = 1, CF_PAD_REFLECT = 2, CF_PAD_SYMMETRIC = 3;

template <int MODE>
__device__ __forceinline__ int cf_pad_map(int s, int n) {
    if (s >= 0 && s < n) return s;
    if constexpr (MODE == CF_PAD_CONSTANT) return -1;
    const int m = MODE == CF_PAD_EDGE ? s : MODE == CF_PAD_REFLECT ? (s < 0 ? -s : 2 * (n - 1) - s) : (s < 0 ? -s - 1 : 2 * n - 1 - s);
    return min(max(m, 0), n - 1);                                          // edge's map; a no-op for pads within the mode's limit
}

// cf_copy_window when the window may leave the image: the block's destination is the same contiguous run of nrows * tw floats,
// its source the nrows x tw window whose first element is (row0, left) of the h x w image at `plane` (line pitch Ws), in the
// image's own coordinates: row0 and left may be negative and the window may end past h / w.  Every source coordinate goes
// through cf_pad_map against (h, w), so no address outside the h x w extent is formed in any mode, and an element of
// constant padding loads nothing: it is fill.  Thread -> element mapping, the (q, rem) stepping, the CF_BATCH loads in flight
// and the stores are cf_copy_window's.  VEC: the group's 4 source columns are the wide ascending load of cf_copy_window when
// all 4 lie in [0, w) (the line inside [0, h) or mapped there); a group that touches a border takes up to 4 mapped single loads.
// Border and interior lanes of a wave diverge there; the interior branch is the unpadded body, and NEITHER branch consumes a
// loaded register: the loads go into raw groups (Load::raw), and decoding (the byte table), mirroring and the stores follow
// once all CF_BATCH groups are issued — with the mirror or the table lookup inside the branches every group waited for its own
// loads.
// The caller guarantees: h, w >= 1; for reflect every pad <= extent - 1 and for symmetric <= extent on its axis (one
// reflection suffices), with row0 >= -pad_top, row0 + nrows <= h + pad_bottom and likewise for left.
template <bool VEC, int MODE, typename Src, typename Load = cf_load_f32>
__device__ __forceinline__ void cf_copy_window_pad(Src plane, int Ws, int h, int w, int row0, int left, float fill,
                                                   float* __restrict__ dst, unsigned total, int tw, int flip, Load load = Load()) {
    constexpr int W = VEC ? 4 : 1;                                         // output columns per access
    const int q = (CF_BLOCK * W) / tw, rem = (CF_BLOCK * W) % tw;
    int yy = (int)(threadIdx.x * W) / tw;
    int x = (int)(threadIdx.x * W) - yy * tw;
    for (unsigned e = threadIdx.x * W; e < total; e += CF_BATCH * CF_BLOCK * W) {
        typename Load::template raw<W> a[CF_BATCH];
#pragma unroll
        for (int k = 0; k < CF_BATCH; ++k) {                               // all loads in flight before the first store
            if (e + (unsigned)k * CF_BLOCK * W < total) {
                const int r = cf_pad_map<MODE>(row0 + yy, h);
                const int c0 = left + (flip ? tw - W - x : x);             // the group's lowest source column
                if (r >= 0 && c0 >= 0 && c0 + W <= w) {
                    load.fetch(plane + (size_t)r * Ws + c0, a[k]);         // ascending addresses; mirrored in registers
                } else {
                    load.begin_singles(a[k]);
#pragma unroll
                    for (int j = 0; j < W; ++j) {
                        const int c = cf_pad_map<MODE>(c0 + j, w);
                        if constexpr (MODE == CF_PAD_CONSTANT) {           // the only mode whose maps say "nowhere"
                            load.set_fill(a[k], j, fill);
                            if (r >= 0 && c >= 0) load.fetch_one(plane + (size_t)r * Ws + c, a[k], j);
                        } else {
                            load.fetch_one(plane + (size_t)r * Ws + c, a[k], j);
                        }
                    }
                }
            }
            x += rem;
            yy += q;
            if (x >= tw) { x -= tw; ++yy; }
        }
#pragma unroll
        for (int k = 0; k < CF_BATCH; ++k) {
            const unsigned i = e + (unsigned)k * CF_BLOCK * W;
            if (i < total) {
                float s[W], v[W];
#pragma unroll
                for (int j = 0; j < W; ++j) s[j] = load.value(a[k], j, fill);
#pragma unroll
                for (int j = 0; j < W; ++j) v[j] = flip ? s[W - 1 - j] : s[j];
                if constexpr (VEC) *reinterpret_cast<float4*>(dst + i) = make_float4(v[0], v[1], v[2], v[3]);
                else dst[i] = v[0];
            }
        }
    }
}
