// Rehearsal baselines (rehearsal/model/baseline_rehearsal_partial_mem.py:125-253): the step's batch assembly, which (with
// the segmented loss of loss.hip) lets one engine pass over [current batch | exemplar chunks] replace the reference's one
// forward / backward per exemplar chunk plus one for the current batch.
//   rehearsal_assemble             the store holds rows of the net's input shape
//   rehearsal_assemble_crop_flip   the store holds FRAMES (the counterpart of the reference's memory of paths: :215-216 rebuilds
//                                  the exemplar loader with the task's train transform at every step); the gathered exemplars
//                                  are cropped and mirrored in the same launch
//   rehearsal_assemble_crop_flip_u8  the same with BYTE frames in the store (clhip.h, byte frames): the ring rows are raw byte
//                                  copies, the gathered exemplars are decoded through the table where they are loaded
//   rehearsal_assemble_resized_crop_flip[_u8]  the train transform is RandomResizedCrop + flip: the gathered exemplars are
//                                  RESAMPLED in the same launch, by the block body of the loaders' resizing gather
//   rehearsal_assemble_pad_crop_flip[_u8]  the train transform is RandomCrop(size, padding, fill, padding_mode) + flip: the
//                                  gathered exemplars are windows of their PADDED frames, by the block body of the loaders'
//                                  padded gather
#include "resized_crop.hpp"
#include <type_traits>

namespace {

constexpr int ASM_BLOCK = 256;
constexpr int ASM_VEC_PER_THREAD = 12;    // float4 per thread, all in flight at once: 48 KB per block = one 3x64x64 row
constexpr size_t ASM_SEG = (size_t)ASM_BLOCK * ASM_VEC_PER_THREAD * 4;       // floats per block
constexpr size_t ASM_SEG_U8 = (size_t)ASM_BLOCK * ASM_VEC_PER_THREAD * 16;   // bytes per block: the same 48 KB
constexpr int ASM_BYTES_PER_THREAD = 16;  // byte accesses per thread in flight at once on the plain byte path
static_assert(ASM_BLOCK == CF_BLOCK, "the crop rows of rehearsal_assemble_cf_kernel run cf_copy_window");

template <typename T> constexpr size_t asm_seg = std::is_same<T, uint8_t>::value ? ASM_SEG_U8 : ASM_SEG;   // elements per block

// Segment `seg` (asm_seg<T> elements = 48 KB, the last one shorter) of a row of `elems` elements, src -> dst.
// VEC: 16-byte accesses (elems * sizeof(T) % 16 == 0, both rows 16-byte aligned: decided on the host).  Otherwise element
// accesses; a byte row of odd size starts at any address, so its plain path is byte loads and byte stores.
template <bool VEC, typename T>
__device__ __forceinline__ void copy_segment(const T* src, T* dst, size_t elems, unsigned seg) {
    if (VEC) {
        const size_t nvec = elems / (16 / sizeof(T));
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        const size_t base = (size_t)seg * ASM_BLOCK * ASM_VEC_PER_THREAD + threadIdx.x;
        float4 v[ASM_VEC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < ASM_VEC_PER_THREAD; ++k) {          // all loads in flight before the first store
            const size_t i = base + (size_t)k * ASM_BLOCK;
            if (i < nvec) v[k] = s4[i];
        }
#pragma unroll
        for (int k = 0; k < ASM_VEC_PER_THREAD; ++k) {
            const size_t i = base + (size_t)k * ASM_BLOCK;
            if (i < nvec) d4[i] = v[k];
        }
    } else if constexpr (std::is_same<T, uint8_t>::value) {
        const size_t end = min(elems, ((size_t)seg + 1) * asm_seg<T>);
        for (size_t i0 = (size_t)seg * asm_seg<T> + threadIdx.x; i0 < end; i0 += (size_t)ASM_BYTES_PER_THREAD * ASM_BLOCK) {
            uint8_t v[ASM_BYTES_PER_THREAD];
#pragma unroll
            for (int k = 0; k < ASM_BYTES_PER_THREAD; ++k) {    // a batch of loads in flight before its first store
                const size_t i = i0 + (size_t)k * ASM_BLOCK;
                if (i < end) v[k] = src[i];
            }
#pragma unroll
            for (int k = 0; k < ASM_BYTES_PER_THREAD; ++k) {
                const size_t i = i0 + (size_t)k * ASM_BLOCK;
                if (i < end) dst[i] = v[k];
            }
        }
    } else {
        const size_t end = min(elems, ((size_t)seg + 1) * asm_seg<T>);
        for (size_t i = (size_t)seg * asm_seg<T> + threadIdx.x; i < end; i += ASM_BLOCK) dst[i] = src[i];
    }
}

// One block row per destination row (blockIdx.y), blockIdx.x walks the row in 48 KB segments.
//   rows [0, B)            x[r]                 -> x_mix[r],          y[r]        -> y_mix[r]
//   rows [B, B + eff)      x[i]                 -> store_x[row0 + i], y[i]        -> store_y[row0 + i]   (ring buffer)
//   rows [B + eff, ...)    store_x[gather[e]]   -> x_mix[B + e],      store_y[..] -> y_mix[B + e]
// A gather index outside [0, store_rows) copies nothing and writes label -1 (the caller's plan never produces one).
template <bool VEC>
__global__ __launch_bounds__(ASM_BLOCK) void rehearsal_assemble_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ y, int B, size_t row_elems, float* store_x, int64_t* store_y,
    long store_rows, long row0, int eff, const int* __restrict__ gather, int E, float* __restrict__ x_mix,
    int64_t* __restrict__ y_mix) {
    const int r = blockIdx.y;
    const float* src;
    float* dst;
    const int64_t* ysrc;
    int64_t* ydst;
    if (r < B) {
        src = x + (size_t)r * row_elems; dst = x_mix + (size_t)r * row_elems;
        ysrc = y + r; ydst = y_mix + r;
    } else if (r < B + eff) {
        const int i = r - B;
        src = x + (size_t)i * row_elems; dst = store_x + (size_t)(row0 + i) * row_elems;
        ysrc = y + i; ydst = store_y + row0 + i;
    } else {
        const int e = r - B - eff;
        const long g = gather[e];
        dst = x_mix + (size_t)(B + e) * row_elems;
        ydst = y_mix + B + e;
        if (g < 0 || g >= store_rows) {
            if (blockIdx.x == 0 && threadIdx.x == 0) *ydst = -1;
            return;
        }
        src = store_x + (size_t)g * row_elems;
        ysrc = store_y + g;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *ydst = *ysrc;
    copy_segment<VEC>(src, dst, row_elems, blockIdx.x);
}

// The frame-mode assembly: the store rows are frames [C][Hs][Ws], x / x_mix rows are [C][th][tw].  A 1-D grid of three runs of
// blocks, each row of a run taking the blocks its own role needs (the roles differ in size: a 3 x 256 x 256 frame is 16
// segments, its 224 x 224 crop 39 windows):
//   copy_rows x row_blocks     x[r]                       -> x_mix[r],            y[r]       -> y_mix[r]     48 KB segments
//   ring x frame_blocks        src_frames[src_idx[i]]     -> store[row0 + i],     y[i]       -> store_y[..]  48 KB segments
//   E x crop_blocks            window of store[gather[e]] -> x_mix[B + e],        store_y[..] -> y_mix[B + e]
// with the window x_mix[B + e][c][y][x] = store[g][c][top + y][left + (flip ? tw - 1 - x : x)] copied as augment.hip copies it:
// one block per (channel, chunk of rpb output lines), everything that selects the source block-uniform (scalar loads, the
// divisions on the scalar unit), lanes along the output line.
// Nothing outside a frame is addressed: a src_idx outside [0, src_rows) leaves its store row as it is and writes store label
// -1; a gather row outside [0, store_rows), top outside [0, Hs - th], left outside [0, Ws - tw] or flip outside {0, 1} copies
// nothing and writes label -1 (the host draws valid tables; this only keeps a bad one from faulting).
// T: the element type of the frames (src_frames, store): float, or uint8_t for a byte store.  A stored byte v of channel c means
// lut[c][v] (clhip.h, byte frames): the ring rows copy bytes, the crop rows decode them where they are loaded, through the block's
// channel of the table staged in LDS (augment.hip), and everything after the load is the float code.
template <typename T>
struct assemble_cf_args {
    const float* x; const int64_t* y; int B, copy_rows;                        // copy_rows = B, or 0 without x_mix
    int C, Hs, Ws, th, tw;
    const float* lut;                                                          // [C][256], byte frames only
    const T* src_frames; long src_rows; const int64_t* src_idx;
    T* store; int64_t* store_y; long store_rows, row0; int ring;
    const int* gather; const int* params; int E;
    float* x_mix; int64_t* y_mix;
    unsigned row_blocks, frame_blocks, crop_blocks;                            // blocks per row of each run
    int rpb, chunks;                                                           // crop_blocks = C * chunks, rpb lines each
    int nb, wmax, ktx, kty;                                                    // the rest of the rz_plan (resized entries only)
    int vec_row, vec_frame;                                                    // 16-byte copies of the two full-row roles
};

// The copy and ring runs of the 1-D grid, shared by the frame-mode kernels.  True: block b served one of them; false: b is now
// the block's number inside the exemplar run.  Block-uniform.
template <typename T>
__device__ __forceinline__ bool assemble_copy_ring(const assemble_cf_args<T>& a, unsigned& b) {
    const size_t row_elems = (size_t)a.C * a.th * a.tw, frame_elems = (size_t)a.C * a.Hs * a.Ws;
    const unsigned n_row = (unsigned)a.copy_rows * a.row_blocks, n_ring = (unsigned)a.ring * a.frame_blocks;
    if (b < n_row) {
        const unsigned r = b / a.row_blocks;
        const unsigned seg = b - r * a.row_blocks;
        if (seg == 0 && threadIdx.x == 0) a.y_mix[r] = a.y[r];
        if (a.vec_row) copy_segment<true>(a.x + r * row_elems, a.x_mix + r * row_elems, row_elems, seg);
        else copy_segment<false>(a.x + r * row_elems, a.x_mix + r * row_elems, row_elems, seg);
        return true;
    }
    b -= n_row;
    if (b < n_ring) {
        const unsigned i = b / a.frame_blocks;
        const unsigned seg = b - i * a.frame_blocks;
        const int64_t s = a.src_idx[i];
        int64_t* ydst = a.store_y + a.row0 + i;
        if (s < 0 || s >= a.src_rows) {
            if (seg == 0 && threadIdx.x == 0) *ydst = -1;
            return true;
        }
        if (seg == 0 && threadIdx.x == 0) *ydst = a.y[i];
        const T* src = a.src_frames + (size_t)s * frame_elems;
        T* dst = a.store + (size_t)(a.row0 + i) * frame_elems;
        if (a.vec_frame) copy_segment<true>(src, dst, frame_elems, seg);
        else copy_segment<false>(src, dst, frame_elems, seg);
        return true;
    }
    b -= n_ring;
    return false;
}

template <bool VEC_CROP, typename T>
__global__ __launch_bounds__(ASM_BLOCK) void rehearsal_assemble_cf_kernel(const assemble_cf_args<T> a) {
    unsigned b = blockIdx.x;
    if (assemble_copy_ring(a, b)) return;
    // (the role and the bad-row test are block-uniform: every thread of a block reaches the barrier below or none does)
    const unsigned e = b / a.crop_blocks;
    const int k = (int)(b - e * a.crop_blocks);
    const long g = a.gather[e];
    const int top = a.params[3 * e], left = a.params[3 * e + 1], flip = a.params[3 * e + 2];
    int64_t* ydst = a.y_mix + a.B + e;
    if (g < 0 || g >= a.store_rows || top < 0 || top > a.Hs - a.th || left < 0 || left > a.Ws - a.tw || (flip != 0 && flip != 1)) {
        if (k == 0 && threadIdx.x == 0) *ydst = -1;
        return;
    }
    if (k == 0 && threadIdx.x == 0) *ydst = a.store_y[g];
    const int c = k / a.chunks;
    const int y0 = (k - c * a.chunks) * a.rpb;
    const int nrows = min(a.rpb, a.th - y0);
    const T* src = a.store + ((size_t)g * a.C + c) * a.Hs * a.Ws + (size_t)(top + y0) * a.Ws + left;
    float* dst = a.x_mix + (((size_t)(a.B + e) * a.C + c) * a.th + y0) * a.tw;
    if constexpr (std::is_same<T, uint8_t>::value) {
        __shared__ float lut_s[256];                                           // the table of channel c (CF_BLOCK == 256: one entry each)
        lut_s[threadIdx.x] = a.lut[c * 256 + (int)threadIdx.x];
        __syncthreads();
        typedef const uint8_t __attribute__((address_space(1))) gbyte;       // (device memory: global_load, not flat_load)
        cf_copy_window<VEC_CROP>((gbyte*)src, a.Ws, dst, (unsigned)nrows * (unsigned)a.tw, a.tw, flip, cf_load_u8{lut_s});
    } else {
        cf_copy_window<VEC_CROP>(src, a.Ws, dst, (unsigned)nrows * (unsigned)a.tw, a.tw, flip);   // total <= max(CF_SEG, tw) < 2^31
    }
}

// The frame-mode assembly under RandomResizedCrop + flip: the grid and the copy / ring runs of rehearsal_assemble_cf_kernel; the
// exemplar run is E x (C * chunks) blocks of the launch's rz_plan, each resampling the (top, left, h, w) window of
// store[gather[e]] to rpb output lines of x_mix[B + e] by rz_resample_block (resized_crop.hpp), the block body of
// gather_resized_kernel (augment.hip): bitwise that gather's result for the same frame and window.  params: int32[E][5] of
// (top, left, h, w, flip).  The launch's dynamic LDS is the plan's (the copy and ring blocks carry it unused).
// A gather row outside [0, store_rows), h < 1, w < 1, top < 0, left < 0, top + h > Hs, left + w > Ws, flip outside {0, 1},
// h > CLHIP_RESIZE_MAX_RATIO th or w > CLHIP_RESIZE_MAX_RATIO tw copies nothing and writes label -1 (the gather's rule); no
// address outside a frame is formed.
template <bool VEC, typename T>
__global__ __launch_bounds__(ASM_BLOCK) void rehearsal_assemble_rz_kernel(const assemble_cf_args<T> a) {
    extern __shared__ __attribute__((aligned(16))) float asm_rz_lds[];
    unsigned b = blockIdx.x;
    if (assemble_copy_ring(a, b)) return;
    // (the role and the bad-row test are block-uniform: every thread of a block reaches the body's barriers or none does)
    const unsigned e = b / a.crop_blocks;
    const int k = (int)(b - e * a.crop_blocks);
    const long g = a.gather[e];
    const int top = a.params[5 * e], left = a.params[5 * e + 1], h = a.params[5 * e + 2], w = a.params[5 * e + 3],
              flip = a.params[5 * e + 4];
    int64_t* ydst = a.y_mix + a.B + e;
    if (g < 0 || g >= a.store_rows || h < 1 || w < 1 || top < 0 || left < 0 || top > a.Hs - h || left > a.Ws - w ||
        (flip != 0 && flip != 1) || (int64_t)h > (int64_t)CLHIP_RESIZE_MAX_RATIO * a.th ||
        (int64_t)w > (int64_t)CLHIP_RESIZE_MAX_RATIO * a.tw) {
        if (k == 0 && threadIdx.x == 0) *ydst = -1;
        return;
    }
    if (k == 0 && threadIdx.x == 0) *ydst = a.store_y[g];
    const int c = k / a.chunks;
    const int y0 = (k - c * a.chunks) * a.rpb;
    const int nrows = min(a.rpb, a.th - y0);
    constexpr bool U8 = std::is_same<T, uint8_t>::value;
    typedef const T __attribute__((address_space(1))) gelem;                   // (device memory: global_load, not flat_load)
    gelem* plane = (gelem*)(a.store + ((size_t)g * a.C + c) * a.Hs * a.Ws);
    const float* lut_c = nullptr;
    if constexpr (U8) lut_c = a.lut + c * 256;
    rz_resample_block<VEC, U8>(asm_rz_lds, plane, a.Ws, top, left, h, w, flip, a.th, a.tw, y0, nrows, a.rpb, a.nb, a.wmax, a.ktx,
                               a.kty, lut_c, a.x_mix + (((size_t)(a.B + e) * a.C + c) * a.th + y0) * a.tw);
}

// The frame-mode assembly under RandomCrop(size, padding, fill, padding_mode) + flip: the grid and the copy / ring runs of
// rehearsal_assemble_cf_kernel; the exemplar run is E x (C * chunks) blocks, each copying rpb = cf_rows_per_block(tw) output
// lines of the window of store[gather[e]]'s PADDED image by cf_copy_window_pad (crop_flip.hpp), the block body of
// gather_pad_crop_flip_kernel (augment.hip): bitwise that gather's result for the same frame and params.  params: int32[E][5] of
// (top, left, flip, h, w), the corner in the frame's unpadded coordinates, (h, w) its valid extent; fill: float[C], output domain.
// A gather row outside [0, store_rows) or a row that gather lists as bad (flip outside {0, 1}, h outside [1, Hs], w outside
// [1, Ws], top outside [-pt, h + pb - th], left outside [-pl, w + pr - tw], pads over the mode's limit for (h, w)) copies nothing
// and writes label -1 (64-bit compares: a bad table may hold any int32); every source coordinate is mapped into the h x w extent,
// so no address outside it is formed.  MODE (the padding mode) is a template argument, as in augment.hip.
template <typename T>
struct assemble_pad_args {
    assemble_cf_args<T> a;
    int pl, pt, pr, pb;
    const float* fill;                                                         // [C]
};

template <bool VEC, int MODE, typename T>
__global__ __launch_bounds__(ASM_BLOCK) void rehearsal_assemble_pad_kernel(const assemble_pad_args<T> p) {
    const assemble_cf_args<T>& a = p.a;
    unsigned b = blockIdx.x;
    if (assemble_copy_ring(a, b)) return;
    // (the role and the bad-row test are block-uniform: every thread of a block reaches the barrier below or none does)
    const unsigned e = b / a.crop_blocks;
    const int k = (int)(b - e * a.crop_blocks);
    const long g = a.gather[e];
    const int top = a.params[5 * e], left = a.params[5 * e + 1], flip = a.params[5 * e + 2], h = a.params[5 * e + 3],
              w = a.params[5 * e + 4];
    int64_t* ydst = a.y_mix + a.B + e;
    constexpr int lim = MODE == CF_PAD_REFLECT ? 1 : 0;                        // reflect: pad <= extent - 1, symmetric: pad <= extent
    const bool one_reflection = MODE < CF_PAD_REFLECT || (max(p.pl, p.pr) <= w - lim && max(p.pt, p.pb) <= h - lim);
    if (g < 0 || g >= a.store_rows || (flip != 0 && flip != 1) || h < 1 || h > a.Hs || w < 1 || w > a.Ws || top < -p.pt ||
        (int64_t)top > (int64_t)h + p.pb - a.th || left < -p.pl || (int64_t)left > (int64_t)w + p.pr - a.tw || !one_reflection) {
        if (k == 0 && threadIdx.x == 0) *ydst = -1;
        return;
    }
    if (k == 0 && threadIdx.x == 0) *ydst = a.store_y[g];
    const int c = k / a.chunks;
    const int y0 = (k - c * a.chunks) * a.rpb;
    const int nrows = min(a.rpb, a.th - y0);
    float* dst = a.x_mix + (((size_t)(a.B + e) * a.C + c) * a.th + y0) * a.tw;
    const float fill_c = p.fill[c];
    typedef const T __attribute__((address_space(1))) gelem;                   // (device memory: global_load, not flat_load)
    gelem* plane = (gelem*)(a.store + ((size_t)g * a.C + c) * a.Hs * a.Ws);
    if constexpr (std::is_same<T, uint8_t>::value) {
        __shared__ float lut_s[257];                                           // the table of channel c (CF_BLOCK == 256: one entry each)
        lut_s[threadIdx.x] = a.lut[c * 256 + (int)threadIdx.x];
        if (threadIdx.x == 0) lut_s[256] = fill_c;                             // entry 256: what a fill element decodes to
        __syncthreads();
        cf_copy_window_pad<VEC, MODE>(plane, a.Ws, h, w, top + y0, left, fill_c, dst, (unsigned)nrows * (unsigned)a.tw, a.tw, flip,
                                      cf_load_u8{lut_s});
    } else {
        cf_copy_window_pad<VEC, MODE>(plane, a.Ws, h, w, top + y0, left, fill_c, dst, (unsigned)nrows * (unsigned)a.tw, a.tw, flip);
    }
}

}  // namespace

// What the padded entries add to the frame-mode arguments.
struct assemble_pad { int mode, pl, pt, pr, pb; const float* fill; };

// One body for the frame-mode entries: T selects the frames' element type, lut is NULL for floats; RESIZED: gather_params rows
// are (top, left, h, w, flip) and the exemplar run resamples, under a plan made here for the frame (needed only with E > 0).
// pad (never with RESIZED): gather_params rows are (top, left, flip, h, w) and the exemplar run copies windows of the padded frames.
template <typename T, bool RESIZED>
static int assemble_frames(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                           const float* lut, const T* src_frames, long src_rows, const int64_t* src_idx, T* store_frames,
                           int64_t* store_labels, long store_rows, long ring_row0, int ring_rows, const int* gather_rows,
                           const int* gather_params, int E, float* x_mix, int64_t* labels_mix, void* stream,
                           const assemble_pad* pad = nullptr) {
    if (B < 0 || E < 0 || ring_rows < 0 || store_rows < 0 || src_rows < 0) return CLHIP_EINVAL;
    if (C < 1 || th < 1 || tw < 1 || Hs < 1 || Ws < 1) return CLHIP_EINVAL;
    if (!RESIZED && !pad && (th > Hs || tw > Ws)) return CLHIP_EINVAL;           // (a resized window may be enlarged, a padded image larger)
    if (pad) {
        if (Hs > CLHIP_PAD_MAX_EXTENT || Ws > CLHIP_PAD_MAX_EXTENT) return CLHIP_EINVAL;   // (2 n - 1 - s stays an int)
        if (pad->mode < CF_PAD_CONSTANT || pad->mode > CF_PAD_SYMMETRIC) return CLHIP_EINVAL;
        if (pad->pl < 0 || pad->pt < 0 || pad->pr < 0 || pad->pb < 0 || pad->pl > CLHIP_PAD_MAX || pad->pt > CLHIP_PAD_MAX ||
            pad->pr > CLHIP_PAD_MAX || pad->pb > CLHIP_PAD_MAX)
            return CLHIP_EINVAL;
        if (E > 0 && !pad->fill) return CLHIP_EINVAL;                            // (a ring-only call pads nothing)
    }
    if (ring_rows > B) return CLHIP_EINVAL;                                      // ring rows are a prefix of the batch
    if (E > 0 && (!x_mix || !gather_rows || !gather_params)) return CLHIP_EINVAL;
    if (std::is_same<T, uint8_t>::value && E > 0 && !lut) return CLHIP_EINVAL;   // (a ring-only call decodes nothing)
    const int copy_rows = x_mix ? B : 0;                                         // no x_mix (E == 0): the ring update alone
    if (copy_rows > 0 && !x) return CLHIP_EINVAL;
    if ((copy_rows > 0 || ring_rows > 0) && !labels_i64) return CLHIP_EINVAL;
    if ((copy_rows > 0 || E > 0) && !labels_mix) return CLHIP_EINVAL;
    if (ring_rows > 0 && (!src_frames || !src_idx)) return CLHIP_EINVAL;
    if ((ring_rows > 0 || E > 0) && (!store_frames || !store_labels)) return CLHIP_EINVAL;
    if (ring_rows > 0 && (ring_row0 < 0 || ring_row0 + ring_rows > store_rows)) return CLHIP_EINVAL;
    const long rows = (long)copy_rows + ring_rows + E;
    if (rows == 0) return 0;
    if (rows > 65535) return CLHIP_EINVAL;
    const size_t row_elems = (size_t)C * th * tw, frame_elems = (size_t)C * Hs * Ws;
    assemble_cf_args<T> a;
    a.x = x; a.y = labels_i64; a.B = B; a.copy_rows = copy_rows;
    a.C = C; a.Hs = Hs; a.Ws = Ws; a.th = th; a.tw = tw;
    a.lut = lut;
    a.src_frames = src_frames; a.src_rows = src_rows; a.src_idx = src_idx;
    a.store = store_frames; a.store_y = store_labels; a.store_rows = store_rows; a.row0 = ring_row0; a.ring = ring_rows;
    a.gather = gather_rows; a.params = gather_params; a.E = E;
    a.x_mix = x_mix; a.y_mix = labels_mix;
    a.rpb = cf_rows_per_block(tw);
    a.chunks = (th + a.rpb - 1) / a.rpb;
    a.nb = a.wmax = a.ktx = a.kty = 0;
    size_t lds = 0;
    if (RESIZED && E > 0) {
        rz_plan p;
        if (!rz_make_plan(Hs, Ws, th, tw, std::is_same<T, uint8_t>::value ? 256 * sizeof(float) : 0, &p)) return CLHIP_ENOTSUP;
        a.rpb = p.rpb; a.chunks = p.chunks; a.nb = p.nb; a.wmax = p.wmax; a.ktx = p.ktx; a.kty = p.kty;
        lds = p.lds;
    }
    const size_t row_blocks = (row_elems + ASM_SEG - 1) / ASM_SEG, frame_blocks = (frame_elems + asm_seg<T> - 1) / asm_seg<T>;
    const size_t crop_blocks = (size_t)C * a.chunks;
    const size_t blocks = copy_rows * row_blocks + ring_rows * frame_blocks + E * crop_blocks;
    if (row_blocks > 0xffffu || frame_blocks > 0xffffu || crop_blocks > 0xffffu || blocks > 0x7fffffffull) return CLHIP_EINVAL;
    a.row_blocks = (unsigned)row_blocks; a.frame_blocks = (unsigned)frame_blocks; a.crop_blocks = (unsigned)crop_blocks;
    a.vec_row = row_elems % 4 == 0 && aligned16(x) && aligned16(x_mix);
    a.vec_frame = (frame_elems * sizeof(T)) % 16 == 0 && aligned16(src_frames) && aligned16(store_frames);
    const bool vec = tw % 4 == 0 && aligned16(x_mix);
    const dim3 grid((unsigned)blocks), block(ASM_BLOCK);
    if (pad) {
        const assemble_pad_args<T> p{a, pad->pl, pad->pt, pad->pr, pad->pb, pad->fill};
#define CLHIP_PAD_LAUNCH(VEC, MODE) \
    hipLaunchKernelGGL((rehearsal_assemble_pad_kernel<VEC, MODE, T>), grid, block, 0, as_stream(stream), p)
        switch (pad->mode) {
        case CF_PAD_CONSTANT: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_CONSTANT); else CLHIP_PAD_LAUNCH(false, CF_PAD_CONSTANT); break;
        case CF_PAD_EDGE: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_EDGE); else CLHIP_PAD_LAUNCH(false, CF_PAD_EDGE); break;
        case CF_PAD_REFLECT: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_REFLECT); else CLHIP_PAD_LAUNCH(false, CF_PAD_REFLECT); break;
        default: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_SYMMETRIC); else CLHIP_PAD_LAUNCH(false, CF_PAD_SYMMETRIC); break;
        }
#undef CLHIP_PAD_LAUNCH
    } else if constexpr (RESIZED) {
        if (vec) hipLaunchKernelGGL((rehearsal_assemble_rz_kernel<true, T>), grid, block, lds, as_stream(stream), a);
        else hipLaunchKernelGGL((rehearsal_assemble_rz_kernel<false, T>), grid, block, lds, as_stream(stream), a);
    } else {
        if (vec) hipLaunchKernelGGL((rehearsal_assemble_cf_kernel<true, T>), grid, block, 0, as_stream(stream), a);
        else hipLaunchKernelGGL((rehearsal_assemble_cf_kernel<false, T>), grid, block, 0, as_stream(stream), a);
    }
    CLHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int clhip_rehearsal_assemble(const float* x, const int64_t* labels_i64, int B, size_t row_elems, float* store_x,
                             int64_t* store_labels, long store_rows, long ring_row0, int ring_rows, const int* gather_rows,
                             int E, float* x_mix, int64_t* labels_mix, void* stream) {
    if (B < 0 || E < 0 || ring_rows < 0 || row_elems == 0 || store_rows < 0) return CLHIP_EINVAL;
    if (ring_rows > B) return CLHIP_EINVAL;                                      // ring rows are a prefix of x
    if ((B > 0 || ring_rows > 0) && (!x || !labels_i64)) return CLHIP_EINVAL;
    if ((B > 0 || E > 0) && (!x_mix || !labels_mix)) return CLHIP_EINVAL;
    if ((ring_rows > 0 || E > 0) && (!store_x || !store_labels)) return CLHIP_EINVAL;
    if (E > 0 && !gather_rows) return CLHIP_EINVAL;
    if (ring_rows > 0 && (ring_row0 < 0 || ring_row0 + ring_rows > store_rows)) return CLHIP_EINVAL;
    const long rows = (long)B + ring_rows + E;
    if (rows == 0) return 0;
    if (rows > 65535) return CLHIP_EINVAL;
    const bool vec = row_elems % 4 == 0 && (!x || aligned16(x)) && (!x_mix || aligned16(x_mix)) && (!store_x || aligned16(store_x));
    dim3 grid((unsigned)((row_elems + ASM_SEG - 1) / ASM_SEG), (unsigned)rows);
    if (vec)
        hipLaunchKernelGGL(rehearsal_assemble_kernel<true>, grid, dim3(ASM_BLOCK), 0, as_stream(stream), x, labels_i64, B, row_elems,
                           store_x, store_labels, store_rows, ring_row0, ring_rows, gather_rows, E, x_mix, labels_mix);
    else
        hipLaunchKernelGGL(rehearsal_assemble_kernel<false>, grid, dim3(ASM_BLOCK), 0, as_stream(stream), x, labels_i64, B, row_elems,
                           store_x, store_labels, store_rows, ring_row0, ring_rows, gather_rows, E, x_mix, labels_mix);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

int clhip_rehearsal_assemble_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                       const float* src_frames, long src_rows, const int64_t* src_idx, float* store_frames,
                                       int64_t* store_labels, long store_rows, long ring_row0, int ring_rows,
                                       const int* gather_rows, const int* gather_params, int E, float* x_mix, int64_t* labels_mix,
                                       void* stream) {
    return assemble_frames<float, false>(x, labels_i64, B, C, Hs, Ws, th, tw, nullptr, src_frames, src_rows, src_idx, store_frames,
                                     store_labels, store_rows, ring_row0, ring_rows, gather_rows, gather_params, E, x_mix,
                                     labels_mix, stream);
}

int clhip_rehearsal_assemble_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                          const float* lut, const uint8_t* src_frames, long src_rows, const int64_t* src_idx,
                                          uint8_t* store_frames, int64_t* store_labels, long store_rows, long ring_row0,
                                          int ring_rows, const int* gather_rows, const int* gather_params, int E, float* x_mix,
                                          int64_t* labels_mix, void* stream) {
    return assemble_frames<uint8_t, false>(x, labels_i64, B, C, Hs, Ws, th, tw, lut, src_frames, src_rows, src_idx, store_frames,
                                       store_labels, store_rows, ring_row0, ring_rows, gather_rows, gather_params, E, x_mix,
                                       labels_mix, stream);
}

int clhip_rehearsal_assemble_resized_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th,
                                               int tw, const float* src_frames, long src_rows, const int64_t* src_idx,
                                               float* store_frames, int64_t* store_labels, long store_rows, long ring_row0,
                                               int ring_rows, const int* gather_rows, const int* gather_params, int E, float* x_mix,
                                               int64_t* labels_mix, void* stream) {
    return assemble_frames<float, true>(x, labels_i64, B, C, Hs, Ws, th, tw, nullptr, src_frames, src_rows, src_idx, store_frames,
                                        store_labels, store_rows, ring_row0, ring_rows, gather_rows, gather_params, E, x_mix,
                                        labels_mix, stream);
}

int clhip_rehearsal_assemble_resized_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th,
                                                  int tw, const float* lut, const uint8_t* src_frames, long src_rows,
                                                  const int64_t* src_idx, uint8_t* store_frames, int64_t* store_labels,
                                                  long store_rows, long ring_row0, int ring_rows, const int* gather_rows,
                                                  const int* gather_params, int E, float* x_mix, int64_t* labels_mix,
                                                  void* stream) {
    return assemble_frames<uint8_t, true>(x, labels_i64, B, C, Hs, Ws, th, tw, lut, src_frames, src_rows, src_idx, store_frames,
                                          store_labels, store_rows, ring_row0, ring_rows, gather_rows, gather_params, E, x_mix,
                                          labels_mix, stream);
}

int clhip_rehearsal_assemble_pad_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                           int mode, int pl, int pt, int pr, int pb, const float* fill, const float* src_frames,
                                           long src_rows, const int64_t* src_idx, float* store_frames, int64_t* store_labels,
                                           long store_rows, long ring_row0, int ring_rows, const int* gather_rows,
                                           const int* gather_params, int E, float* x_mix, int64_t* labels_mix, void* stream) {
    const assemble_pad pad{mode, pl, pt, pr, pb, fill};
    return assemble_frames<float, false>(x, labels_i64, B, C, Hs, Ws, th, tw, nullptr, src_frames, src_rows, src_idx, store_frames,
                                         store_labels, store_rows, ring_row0, ring_rows, gather_rows, gather_params, E, x_mix,
                                         labels_mix, stream, &pad);
}

int clhip_rehearsal_assemble_pad_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th,
                                              int tw, int mode, int pl, int pt, int pr, int pb, const float* fill, const float* lut,
                                              const uint8_t* src_frames, long src_rows, const int64_t* src_idx,
                                              uint8_t* store_frames, int64_t* store_labels, long store_rows, long ring_row0,
                                              int ring_rows, const int* gather_rows, const int* gather_params, int E, float* x_mix,
                                              int64_t* labels_mix, void* stream) {
    const assemble_pad pad{mode, pl, pt, pr, pb, fill};
    return assemble_frames<uint8_t, false>(x, labels_i64, B, C, Hs, Ws, th, tw, lut, src_frames, src_rows, src_idx, store_frames,
                                           store_labels, store_rows, ring_row0, ring_rows, gather_rows, gather_params, E, x_mix,
                                           labels_mix, stream, &pad);
}

}  // extern "C"
