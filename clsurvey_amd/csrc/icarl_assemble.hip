// iCaRL on augmented tasks (rehearsal/model/icarl.py:482-598): the assembly of one update_representation step when the store
// holds FRAMES.  The reference rebuilds the exemplar loader with the task's train transform at every step (:560-561), so a
// replayed exemplar is a fresh crop, and reads the exemplar's distillation target, computed once at herding time (:476-479), by
// its index (:566-574).  Here ONE launch fills the mixed batch: the current rows, the fresh windows of the gathered frames, and
// the stored target rows of the same exemplars (the crop-mode step takes two clhip_rehearsal_assemble launches for that).
//   icarl_assemble_crop_flip[_u8]           RandomCrop + flip: the window is copied by cf_copy_window (crop_flip.hpp)
//   icarl_assemble_resized_crop_flip[_u8]   RandomResizedCrop + flip: the window is resampled by rz_resample_block (resized_crop.hpp)
//   icarl_assemble_pad_crop_flip[_u8]       RandomCrop(size, padding, fill, padding_mode) + flip (datasets/dataset_utils.py's
//                                           CIFAR-style train transform): the store holds the UNPADDED frames and the window of
//                                           the padded image is copied by cf_copy_window_pad (crop_flip.hpp)
// All are the block bodies of the loaders' gathers (augment.hip) and of the rehearsal assembly (rehearsal.hip): bitwise their
// results for the same frame and draw.
#include "resized_crop.hpp"
#include <type_traits>

namespace {

constexpr int IA_BLOCK = 256;
constexpr int IA_VEC_PER_THREAD = 12;     // float4 per thread, all in flight at once: 48 KB per block = one 3x64x64 row
constexpr size_t IA_SEG = (size_t)IA_BLOCK * IA_VEC_PER_THREAD * 4;          // floats per block of the copy run
constexpr int IA_TGT_PER_THREAD = 4;      // accesses per thread of the target run, loads first
constexpr size_t IA_TGT_UNITS = (size_t)IA_BLOCK * IA_TGT_PER_THREAD;        // accesses (float4 or float) per target block
static_assert(IA_BLOCK == CF_BLOCK, "the window blocks run cf_copy_window / rz_resample_block");

// Segment `seg` (IA_SEG floats, the last one shorter) of a row of `elems` floats, src -> dst (rehearsal.hip's copy_segment for
// floats).  VEC: elems % 4 == 0 and both rows 16-byte aligned (decided on the host).
template <bool VEC>
__device__ __forceinline__ void ia_copy_segment(const float* __restrict__ src, float* __restrict__ dst, size_t elems, unsigned seg) {
    if (VEC) {
        const size_t nvec = elems / 4;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        const size_t base = (size_t)seg * IA_BLOCK * IA_VEC_PER_THREAD + threadIdx.x;
        float4 v[IA_VEC_PER_THREAD];
#pragma unroll
        for (int k = 0; k < IA_VEC_PER_THREAD; ++k) {           // all loads in flight before the first store
            const size_t i = base + (size_t)k * IA_BLOCK;
            if (i < nvec) v[k] = s4[i];
        }
#pragma unroll
        for (int k = 0; k < IA_VEC_PER_THREAD; ++k) {
            const size_t i = base + (size_t)k * IA_BLOCK;
            if (i < nvec) d4[i] = v[k];
        }
    } else {
        const size_t end = min(elems, ((size_t)seg + 1) * IA_SEG);
        for (size_t i = (size_t)seg * IA_SEG + threadIdx.x; i < end; i += IA_BLOCK) dst[i] = src[i];
    }
}

template <typename T>
struct icarl_asm_args {
    const float* x; const int64_t* y; int B;
    int C, Hs, Ws, th, tw;
    const float* lut;                                                          // [C][256], byte frames only
    const T* store; long store_rows;
    const int* gather; const int* params; int E;
    const float* store_t; int n_outputs;
    float* x_mix; int64_t* y_mix; float* t_mix;
    unsigned row_blocks, crop_blocks;                                          // blocks per row of the first two runs
    int rpb, chunks;                                                           // crop_blocks = C * chunks, rpb lines each
    int nb, wmax, ktx, kty;                                                    // the rest of the rz_plan (resized entries only)
    int vec_row, vec_t;                                                        // 16-byte accesses of the copy / target runs
    int pl, pt, pr, pb;                                                        // the padded entries only
    const float* fill;                                                         // [C], the padded entries only
};

// What a launch's params rows hold: (top, left, flip), (top, left, h, w, flip), or, KIND >= 0, the padded row (top, left, flip,
// h, w) under the padding mode KIND (CF_PAD_*).
constexpr int IA_CROP = -1, IA_RESIZED = -2;

// A draw the window blocks and the target blocks both refuse (the rules of rehearsal_assemble_cf_kernel / ..._rz_kernel /
// ..._pad_kernel).
template <int KIND, typename T>
__device__ __forceinline__ bool ia_bad_row(const icarl_asm_args<T>& a, unsigned e) {
    const long g = a.gather[e];
    if (g < 0 || g >= a.store_rows) return true;
    if constexpr (KIND >= 0) {
        const int top = a.params[5 * e], left = a.params[5 * e + 1], flip = a.params[5 * e + 2], h = a.params[5 * e + 3],
                  w = a.params[5 * e + 4];
        constexpr int lim = KIND == CF_PAD_REFLECT ? 1 : 0;                    // reflect: pad <= extent - 1, symmetric: pad <= extent
        const bool one_reflection = KIND < CF_PAD_REFLECT || (max(a.pl, a.pr) <= w - lim && max(a.pt, a.pb) <= h - lim);
        return (flip != 0 && flip != 1) || h < 1 || h > a.Hs || w < 1 || w > a.Ws || top < -a.pt ||
               (int64_t)top > (int64_t)h + a.pb - a.th || left < -a.pl || (int64_t)left > (int64_t)w + a.pr - a.tw || !one_reflection;
    } else if constexpr (KIND == IA_RESIZED) {
        const int top = a.params[5 * e], left = a.params[5 * e + 1], h = a.params[5 * e + 2], w = a.params[5 * e + 3],
                  flip = a.params[5 * e + 4];
        return h < 1 || w < 1 || top < 0 || left < 0 || top > a.Hs - h || left > a.Ws - w || (flip != 0 && flip != 1) ||
               (int64_t)h > (int64_t)CLHIP_RESIZE_MAX_RATIO * a.th || (int64_t)w > (int64_t)CLHIP_RESIZE_MAX_RATIO * a.tw;
    } else {
        const int top = a.params[3 * e], left = a.params[3 * e + 1], flip = a.params[3 * e + 2];
        return top < 0 || top > a.Hs - a.th || left < 0 || left > a.Ws - a.tw || (flip != 0 && flip != 1);
    }
}

// The copy run.  True: block b served it; false: b is now the block's number behind it.  Block-uniform.
template <typename T>
__device__ __forceinline__ bool ia_copy_run(const icarl_asm_args<T>& a, unsigned& b) {
    const unsigned n_row = (unsigned)a.B * a.row_blocks;
    if (b >= n_row) {
        b -= n_row;
        return false;
    }
    const size_t row_elems = (size_t)a.C * a.th * a.tw;
    const unsigned r = b / a.row_blocks;
    const unsigned seg = b - r * a.row_blocks;
    if (seg == 0 && threadIdx.x == 0) a.y_mix[r] = a.y[r];
    if (a.vec_row) ia_copy_segment<true>(a.x + r * row_elems, a.x_mix + r * row_elems, row_elems, seg);
    else ia_copy_segment<false>(a.x + r * row_elems, a.x_mix + r * row_elems, row_elems, seg);
    return true;
}

// The target run: block b (counted from the run's first block) moves IA_TGT_UNITS accesses of the E x n_outputs target rows,
// store_t[gather[e]] -> t_mix[B + e]; a thread's accesses are IA_BLOCK apart, so a wave's lanes run along a row.  A bad row
// (ia_bad_row, per access: nothing here is block-uniform, and there is no barrier) is left as it is.
template <int KIND, typename T>
__device__ __forceinline__ void ia_target_run(const icarl_asm_args<T>& a, unsigned b) {
    const unsigned per_row = a.vec_t ? (unsigned)a.n_outputs / 4 : (unsigned)a.n_outputs;   // accesses per target row
    const size_t total = (size_t)a.E * per_row;
    const size_t i0 = (size_t)b * IA_TGT_UNITS + threadIdx.x;
    float4 v[IA_TGT_PER_THREAD];
    size_t dst[IA_TGT_PER_THREAD];
    bool ok[IA_TGT_PER_THREAD];
#pragma unroll
    for (int k = 0; k < IA_TGT_PER_THREAD; ++k) {               // all loads in flight before the first store
        const size_t i = i0 + (size_t)k * IA_BLOCK;
        ok[k] = false;
        if (i < total) {
            const unsigned e = (unsigned)(i / per_row);
            const unsigned j = (unsigned)(i - (size_t)e * per_row);
            if (!ia_bad_row<KIND>(a, e)) {
                ok[k] = true;
                const size_t src = (size_t)a.gather[e] * a.n_outputs;
                dst[k] = (size_t)(a.B + e) * a.n_outputs;
                if (a.vec_t) {
                    v[k] = reinterpret_cast<const float4*>(a.store_t + src)[j];
                    dst[k] += 4 * (size_t)j;
                } else {
                    v[k].x = a.store_t[src + j];
                    dst[k] += j;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < IA_TGT_PER_THREAD; ++k) {
        if (ok[k]) {
            if (a.vec_t) *reinterpret_cast<float4*>(a.t_mix + dst[k]) = v[k];
            else a.t_mix[dst[k]] = v[k].x;
        }
    }
}

// Crop + flip.  The window run is rehearsal_assemble_cf_kernel's exemplar run: one block per (exemplar, channel, chunk of rpb
// output lines), everything that selects the source block-uniform, lanes along the output line; byte frames are decoded through
// the block's channel of the table staged in LDS.
template <bool VEC_CROP, typename T>
__global__ __launch_bounds__(IA_BLOCK) void icarl_assemble_cf_kernel(const icarl_asm_args<T> a) {
    unsigned b = blockIdx.x;
    if (ia_copy_run(a, b)) return;
    const unsigned n_crop = (unsigned)a.E * a.crop_blocks;
    if (b >= n_crop) {
        ia_target_run<IA_CROP>(a, b - n_crop);
        return;
    }
    // (the role and the bad-row test are block-uniform: every thread of a block reaches the barrier below or none does)
    const unsigned e = b / a.crop_blocks;
    const int k = (int)(b - e * a.crop_blocks);
    int64_t* ydst = a.y_mix + a.B + e;
    if (ia_bad_row<IA_CROP>(a, e)) {
        if (k == 0 && threadIdx.x == 0) *ydst = -1;
        return;
    }
    if (k == 0 && threadIdx.x == 0) *ydst = 0;
    const long g = a.gather[e];
    const int top = a.params[3 * e], left = a.params[3 * e + 1], flip = a.params[3 * e + 2];
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

// RandomResizedCrop + flip.  The window run is rehearsal_assemble_rz_kernel's exemplar run under the launch's rz_plan; the
// launch's dynamic LDS is the plan's (the copy and target blocks carry it unused).
template <bool VEC, typename T>
__global__ __launch_bounds__(IA_BLOCK) void icarl_assemble_rz_kernel(const icarl_asm_args<T> a) {
    extern __shared__ __attribute__((aligned(16))) float ia_rz_lds[];
    unsigned b = blockIdx.x;
    if (ia_copy_run(a, b)) return;
    const unsigned n_crop = (unsigned)a.E * a.crop_blocks;
    if (b >= n_crop) {
        ia_target_run<IA_RESIZED>(a, b - n_crop);
        return;
    }
    // (the role and the bad-row test are block-uniform: every thread of a block reaches the body's barriers or none does)
    const unsigned e = b / a.crop_blocks;
    const int k = (int)(b - e * a.crop_blocks);
    int64_t* ydst = a.y_mix + a.B + e;
    if (ia_bad_row<IA_RESIZED>(a, e)) {
        if (k == 0 && threadIdx.x == 0) *ydst = -1;
        return;
    }
    if (k == 0 && threadIdx.x == 0) *ydst = 0;
    const long g = a.gather[e];
    const int top = a.params[5 * e], left = a.params[5 * e + 1], h = a.params[5 * e + 2], w = a.params[5 * e + 3],
              flip = a.params[5 * e + 4];
    const int c = k / a.chunks;
    const int y0 = (k - c * a.chunks) * a.rpb;
    const int nrows = min(a.rpb, a.th - y0);
    constexpr bool U8 = std::is_same<T, uint8_t>::value;
    typedef const T __attribute__((address_space(1))) gelem;                   // (device memory: global_load, not flat_load)
    gelem* plane = (gelem*)(a.store + ((size_t)g * a.C + c) * a.Hs * a.Ws);
    const float* lut_c = nullptr;
    if constexpr (U8) lut_c = a.lut + c * 256;
    rz_resample_block<VEC, U8>(ia_rz_lds, plane, a.Ws, top, left, h, w, flip, a.th, a.tw, y0, nrows, a.rpb, a.nb, a.wmax, a.ktx,
                               a.kty, lut_c, a.x_mix + (((size_t)(a.B + e) * a.C + c) * a.th + y0) * a.tw);
}

// RandomCrop(size, padding, fill, padding_mode) + flip.  The window run is rehearsal_assemble_pad_kernel's exemplar run: one
// block per (exemplar, channel, chunk of rpb output lines) copies its lines of the window of store[gather[e]]'s PADDED image by
// cf_copy_window_pad, every source coordinate mapped into the row's own h x w extent; byte frames are decoded through the
// block's channel of the table staged in LDS, entry 256 the decoded fill.  MODE (the padding mode) is a template argument, as
// in augment.hip.
template <bool VEC, int MODE, typename T>
__global__ __launch_bounds__(IA_BLOCK) void icarl_assemble_pad_kernel(const icarl_asm_args<T> a) {
    unsigned b = blockIdx.x;
    if (ia_copy_run(a, b)) return;
    const unsigned n_crop = (unsigned)a.E * a.crop_blocks;
    if (b >= n_crop) {
        ia_target_run<MODE>(a, b - n_crop);
        return;
    }
    // (the role and the bad-row test are block-uniform: every thread of a block reaches the barrier below or none does)
    const unsigned e = b / a.crop_blocks;
    const int k = (int)(b - e * a.crop_blocks);
    int64_t* ydst = a.y_mix + a.B + e;
    if (ia_bad_row<MODE>(a, e)) {
        if (k == 0 && threadIdx.x == 0) *ydst = -1;
        return;
    }
    if (k == 0 && threadIdx.x == 0) *ydst = 0;
    const long g = a.gather[e];
    const int top = a.params[5 * e], left = a.params[5 * e + 1], flip = a.params[5 * e + 2], h = a.params[5 * e + 3],
              w = a.params[5 * e + 4];
    const int c = k / a.chunks;
    const int y0 = (k - c * a.chunks) * a.rpb;
    const int nrows = min(a.rpb, a.th - y0);
    float* dst = a.x_mix + (((size_t)(a.B + e) * a.C + c) * a.th + y0) * a.tw;
    const float fill_c = a.fill[c];
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

// What the padded entries add to the arguments.
struct icarl_pad { int mode, pl, pt, pr, pb; const float* fill; };

// One body for the six entries: T selects the frames' element type, lut is NULL for floats; RESIZED: gather_params rows are
// (top, left, h, w, flip) and the window run resamples, under a plan made here for the frame (needed only with E > 0).
// pad (never with RESIZED): gather_params rows are (top, left, flip, h, w) and the window run copies windows of the padded frames.
template <typename T, bool RESIZED>
static int icarl_assemble(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                          const float* lut, const T* store_frames, long store_rows, const int* gather_rows,
                          const int* gather_params, int E, const float* store_t, int n_outputs, float* x_mix,
                          int64_t* labels_mix, float* t_mix, void* stream, const icarl_pad* pad = nullptr) {
    if (B < 0 || E < 0 || store_rows < 0) return CLHIP_EINVAL;
    if (C < 1 || th < 1 || tw < 1 || Hs < 1 || Ws < 1 || n_outputs < 1) return CLHIP_EINVAL;
    if (!RESIZED && !pad && (th > Hs || tw > Ws)) return CLHIP_EINVAL;           // (a resized window may be enlarged, a padded image larger)
    if (pad) {
        if (Hs > CLHIP_PAD_MAX_EXTENT || Ws > CLHIP_PAD_MAX_EXTENT) return CLHIP_EINVAL;   // (2 n - 1 - s stays an int)
        if (pad->mode < CF_PAD_CONSTANT || pad->mode > CF_PAD_SYMMETRIC) return CLHIP_EINVAL;
        if (pad->pl < 0 || pad->pt < 0 || pad->pr < 0 || pad->pb < 0 || pad->pl > CLHIP_PAD_MAX || pad->pt > CLHIP_PAD_MAX ||
            pad->pr > CLHIP_PAD_MAX || pad->pb > CLHIP_PAD_MAX)
            return CLHIP_EINVAL;
        if (E > 0 && !pad->fill) return CLHIP_EINVAL;                            // (a copy-only call pads nothing)
    }
    if (B > 0 && (!x || !labels_i64 || !x_mix || !labels_mix)) return CLHIP_EINVAL;
    if (E > 0 && (!store_frames || !gather_rows || !gather_params || !store_t || !x_mix || !labels_mix || !t_mix)) return CLHIP_EINVAL;
    if (std::is_same<T, uint8_t>::value && E > 0 && !lut) return CLHIP_EINVAL;
    const long rows = (long)B + E;
    if (rows == 0) return 0;
    if (rows > 65535) return CLHIP_EINVAL;
    const size_t row_elems = (size_t)C * th * tw;
    icarl_asm_args<T> a;
    a.x = x; a.y = labels_i64; a.B = B;
    a.C = C; a.Hs = Hs; a.Ws = Ws; a.th = th; a.tw = tw;
    a.lut = lut;
    a.store = store_frames; a.store_rows = store_rows;
    a.gather = gather_rows; a.params = gather_params; a.E = E;
    a.store_t = store_t; a.n_outputs = n_outputs;
    a.x_mix = x_mix; a.y_mix = labels_mix; a.t_mix = t_mix;
    a.rpb = cf_rows_per_block(tw);
    a.chunks = (th + a.rpb - 1) / a.rpb;
    a.nb = a.wmax = a.ktx = a.kty = 0;
    a.pl = a.pt = a.pr = a.pb = 0; a.fill = nullptr;
    if (pad) { a.pl = pad->pl; a.pt = pad->pt; a.pr = pad->pr; a.pb = pad->pb; a.fill = pad->fill; }
    size_t lds = 0;
    if (RESIZED && E > 0) {
        rz_plan p;
        if (!rz_make_plan(Hs, Ws, th, tw, std::is_same<T, uint8_t>::value ? 256 * sizeof(float) : 0, &p)) return CLHIP_ENOTSUP;
        a.rpb = p.rpb; a.chunks = p.chunks; a.nb = p.nb; a.wmax = p.wmax; a.ktx = p.ktx; a.kty = p.kty;
        lds = p.lds;
    }
    a.vec_row = row_elems % 4 == 0 && aligned16(x) && aligned16(x_mix);
    a.vec_t = n_outputs % 4 == 0 && aligned16(store_t) && aligned16(t_mix);
    const size_t row_blocks = (row_elems + IA_SEG - 1) / IA_SEG, crop_blocks = (size_t)C * a.chunks;
    const size_t t_units = (size_t)E * (a.vec_t ? n_outputs / 4 : n_outputs);
    const size_t t_blocks = (t_units + IA_TGT_UNITS - 1) / IA_TGT_UNITS;
    const size_t blocks = B * row_blocks + E * crop_blocks + t_blocks;
    if (row_blocks > 0xffffu || crop_blocks > 0xffffu || blocks > 0x7fffffffull) return CLHIP_EINVAL;
    a.row_blocks = (unsigned)row_blocks; a.crop_blocks = (unsigned)crop_blocks;
    const bool vec = tw % 4 == 0 && aligned16(x_mix);
    const dim3 grid((unsigned)blocks), block(IA_BLOCK);
    if (pad) {
#define CLHIP_PAD_LAUNCH(VEC, MODE) \
    hipLaunchKernelGGL((icarl_assemble_pad_kernel<VEC, MODE, T>), grid, block, 0, as_stream(stream), a)
        switch (pad->mode) {
        case CF_PAD_CONSTANT: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_CONSTANT); else CLHIP_PAD_LAUNCH(false, CF_PAD_CONSTANT); break;
        case CF_PAD_EDGE: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_EDGE); else CLHIP_PAD_LAUNCH(false, CF_PAD_EDGE); break;
        case CF_PAD_REFLECT: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_REFLECT); else CLHIP_PAD_LAUNCH(false, CF_PAD_REFLECT); break;
        default: if (vec) CLHIP_PAD_LAUNCH(true, CF_PAD_SYMMETRIC); else CLHIP_PAD_LAUNCH(false, CF_PAD_SYMMETRIC); break;
        }
#undef CLHIP_PAD_LAUNCH
    } else if constexpr (RESIZED) {
        if (vec) hipLaunchKernelGGL((icarl_assemble_rz_kernel<true, T>), grid, block, lds, as_stream(stream), a);
        else hipLaunchKernelGGL((icarl_assemble_rz_kernel<false, T>), grid, block, lds, as_stream(stream), a);
    } else {
        if (vec) hipLaunchKernelGGL((icarl_assemble_cf_kernel<true, T>), grid, block, 0, as_stream(stream), a);
        else hipLaunchKernelGGL((icarl_assemble_cf_kernel<false, T>), grid, block, 0, as_stream(stream), a);
    }
    CLHIP_LAUNCH_CHECK();
    return 0;
}

extern "C" {

int clhip_icarl_assemble_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                   const float* store_frames, long store_rows, const int* gather_rows, const int* gather_params,
                                   int E, const float* store_t, int n_outputs, float* x_mix, int64_t* labels_mix, float* t_mix,
                                   void* stream) {
    return icarl_assemble<float, false>(x, labels_i64, B, C, Hs, Ws, th, tw, nullptr, store_frames, store_rows, gather_rows,
                                        gather_params, E, store_t, n_outputs, x_mix, labels_mix, t_mix, stream);
}

int clhip_icarl_assemble_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                      const float* lut, const uint8_t* store_frames, long store_rows, const int* gather_rows,
                                      const int* gather_params, int E, const float* store_t, int n_outputs, float* x_mix,
                                      int64_t* labels_mix, float* t_mix, void* stream) {
    return icarl_assemble<uint8_t, false>(x, labels_i64, B, C, Hs, Ws, th, tw, lut, store_frames, store_rows, gather_rows,
                                          gather_params, E, store_t, n_outputs, x_mix, labels_mix, t_mix, stream);
}

int clhip_icarl_assemble_resized_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                           const float* store_frames, long store_rows, const int* gather_rows,
                                           const int* gather_params, int E, const float* store_t, int n_outputs, float* x_mix,
                                           int64_t* labels_mix, float* t_mix, void* stream) {
    return icarl_assemble<float, true>(x, labels_i64, B, C, Hs, Ws, th, tw, nullptr, store_frames, store_rows, gather_rows,
                                       gather_params, E, store_t, n_outputs, x_mix, labels_mix, t_mix, stream);
}

int clhip_icarl_assemble_resized_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th,
                                              int tw, const float* lut, const uint8_t* store_frames, long store_rows,
                                              const int* gather_rows, const int* gather_params, int E, const float* store_t,
                                              int n_outputs, float* x_mix, int64_t* labels_mix, float* t_mix, void* stream) {
    return icarl_assemble<uint8_t, true>(x, labels_i64, B, C, Hs, Ws, th, tw, lut, store_frames, store_rows, gather_rows,
                                         gather_params, E, store_t, n_outputs, x_mix, labels_mix, t_mix, stream);
}

int clhip_icarl_assemble_pad_crop_flip(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                       int mode, int pl, int pt, int pr, int pb, const float* fill, const float* store_frames,
                                       long store_rows, const int* gather_rows, const int* gather_params, int E,
                                       const float* store_t, int n_outputs, float* x_mix, int64_t* labels_mix, float* t_mix,
                                       void* stream) {
    const icarl_pad pad{mode, pl, pt, pr, pb, fill};
    return icarl_assemble<float, false>(x, labels_i64, B, C, Hs, Ws, th, tw, nullptr, store_frames, store_rows, gather_rows,
                                        gather_params, E, store_t, n_outputs, x_mix, labels_mix, t_mix, stream, &pad);
}

int clhip_icarl_assemble_pad_crop_flip_u8(const float* x, const int64_t* labels_i64, int B, int C, int Hs, int Ws, int th, int tw,
                                          int mode, int pl, int pt, int pr, int pb, const float* fill, const float* lut,
                                          const uint8_t* store_frames, long store_rows, const int* gather_rows,
                                          const int* gather_params, int E, const float* store_t, int n_outputs, float* x_mix,
                                          int64_t* labels_mix, float* t_mix, void* stream) {
    const icarl_pad pad{mode, pl, pt, pr, pb, fill};
    return icarl_assemble<uint8_t, false>(x, labels_i64, B, C, Hs, Ws, th, tw, lut, store_frames, store_rows, gather_rows,
                                          gather_params, E, store_t, n_outputs, x_mix, labels_mix, t_mix, stream, &pad);
}

}  // extern "C"
