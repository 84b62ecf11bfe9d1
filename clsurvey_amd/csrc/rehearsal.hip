// Rehearsal baselines (rehearsal/model/baseline_rehearsal_partial_mem.py:125-253): the step's batch assembly, which (with
// the segmented loss of loss.hip) lets one engine pass over [current batch | exemplar chunks] replace the reference's one
// forward / backward per exemplar chunk plus one for the current batch.
#include "common.hpp"

namespace {

constexpr int ASM_BLOCK = 256;
constexpr int ASM_VEC_PER_THREAD = 12;    // float4 per thread, all in flight at once: 48 KB per block = one 3x64x64 row

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
    if (VEC) {
        const size_t nvec = row_elems / 4;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        const size_t base = (size_t)blockIdx.x * ASM_BLOCK * ASM_VEC_PER_THREAD + threadIdx.x;
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
    } else {
        const size_t seg = (size_t)ASM_BLOCK * ASM_VEC_PER_THREAD * 4;
        const size_t end = min(row_elems, ((size_t)blockIdx.x + 1) * seg);
        for (size_t i = (size_t)blockIdx.x * seg + threadIdx.x; i < end; i += ASM_BLOCK) dst[i] = src[i];
    }
}

}  // namespace

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
    const size_t seg = (size_t)ASM_BLOCK * ASM_VEC_PER_THREAD * 4;
    dim3 grid((unsigned)((row_elems + seg - 1) / seg), (unsigned)rows);
    if (vec)
        hipLaunchKernelGGL(rehearsal_assemble_kernel<true>, grid, dim3(ASM_BLOCK), 0, as_stream(stream), x, labels_i64, B, row_elems,
                           store_x, store_labels, store_rows, ring_row0, ring_rows, gather_rows, E, x_mix, labels_mix);
    else
        hipLaunchKernelGGL(rehearsal_assemble_kernel<false>, grid, dim3(ASM_BLOCK), 0, as_stream(stream), x, labels_i64, B, row_elems,
                           store_x, store_labels, store_rows, ring_row0, ring_rows, gather_rows, E, x_mix, labels_mix);
    CLHIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
